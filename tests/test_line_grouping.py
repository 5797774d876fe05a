"""Host: the statement of the line grouping (glass_amd.postprocess.line_grouping.group_lines_host) against the independent
checker of line_group_cases.py on every case, the stated properties on the valid words, every ValueError, the header, the
config keys, and `lines_of` on hand-made Instances."""
import math
import os

import numpy as np
import pytest

import line_group_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glass_group_lines_workspace_bytes", "glass_group_lines"]
RESERVED = ("glass_ring_simplify", "glass_beam_search_merged", "glass_beam_search_dfa", "glass_beam_search_wdfa", "glass_roi_mask")


def test_equals_the_checker_on_every_case():
    from glass_amd.postprocess.line_grouping import group_lines_host
    multi = 0
    for name, boxes, ref in C.all_cases():
        got = group_lines_host(boxes)
        n = len(boxes)
        print(f"[line_group] {name}: {n} words, {ref['line_count']} lines, {len(ref['links'])} links, margins "
              f"{ref['pair_margin']:.2e} / {ref['key_margin']:.2e}")
        assert got["line_count"] == ref["line_count"], name
        for k in ("line_id", "line_pos", "order", "line_start"):
            assert got[k].dtype == np.int32 and got[k].tolist() == ref[k], (name, k)
        assert got["line_boxes"].dtype == np.float32 and got["line_boxes"].shape == (ref["line_count"], 5), name
        for l in range(ref["line_count"]):
            assert C.box_ulps(got["line_boxes"][l], ref["line_boxes"][l]) <= 1, (name, l)
        multi += ref["line_count"] not in (0, 1, n)
    assert multi >= 8                                                  # not a comparison of trivial groupings


def test_known_answers():
    from glass_amd.postprocess.line_grouping import group_lines_host
    got = group_lines_host(C.bridge())
    assert got["line_count"] == 1 and got["order"].tolist() == [1, 2, 0] and got["line_pos"].tolist() == [2, 0, 1]
    assert got["line_boxes"][0].tolist() == [55.0, 50.0, 150.0, 20.0, 0.0]
    ref = C.case("bridge")[2]
    assert ref["links"] == {(0, 2), (1, 2)}
    got = group_lines_host(C.opposite_lines())
    assert got["line_count"] == 2 and sorted(np.bincount(got["line_id"]).tolist()) == [7, 9]
    boxes = C.opposite_lines()
    for l in range(2):                                                 # each line reads along its own direction
        words = got["order"][got["line_start"][l]:got["line_start"][l + 1]]
        xs = boxes[words, 0]
        assert (np.diff(xs) > 0).all() if boxes[words[0], 4] == 0 else (np.diff(xs) < 0).all()
    got = group_lines_host(C.identical(70))
    assert got["line_count"] == 1 and got["order"].tolist() == list(range(70))
    got = group_lines_host(C.arc(36, 3.75))                            # |D| = 0 up to rounding: the frame of word 0
    assert got["line_count"] == 1 and got["line_boxes"][0, 4] == np.float32(C.arc(36, 3.75)[0, 4])
    got = group_lines_host(C.arc(13))
    assert got["line_count"] == 1 and got["order"].tolist() == list(range(13))
    empty = group_lines_host(np.zeros((0, 5), dtype=np.float32))
    assert empty["line_count"] == 0 and empty["line_start"].tolist() == [0] and empty["line_boxes"].shape == (0, 5)
    # an invalid word is a line of its own, after the valid lines, its box its own values bit for bit
    name, boxes, ref = C.case("words that are no words")
    got = group_lines_host(boxes)
    bad = [k for k in range(len(boxes)) if not ref["valid"][k]]
    assert len(bad) == 9 and got["order"][-9:].tolist() == bad
    for k in bad:
        assert got["line_boxes"][got["line_id"][k]].view(np.uint32).tolist() == boxes[k].view(np.uint32).tolist()


def test_properties_on_the_valid_words():
    from glass_amd.postprocess.line_grouping import group_lines_host
    for name, boxes, ref in C.all_cases():
        n = len(boxes)
        if n > 400:
            continue                                                   # (the pair loops below are quadratic Python)
        got = group_lines_host(boxes)
        rows = [[float(v) for v in r] for r in boxes]
        valid = [C.is_valid(r) for r in rows]
        link = {(i, j) for i in range(n) for j in range(n) if i != j and valid[i] and valid[j] and C.pair_link(rows[i], rows[j])[0]}
        assert all((j, i) in link for i, j in link), name                                       # symmetric
        lid = got["line_id"].tolist()
        assert all(lid[i] == lid[j] for i, j in link), name                                     # no link between two lines
        assert sorted(got["order"].tolist()) == list(range(n)), name                            # a permutation
        L = got["line_count"]
        start = got["line_start"].tolist()
        assert start[0] == 0 and start[L] == n and all(a < b for a, b in zip(start[:-1], start[1:])), name
        for l in range(L):
            words = got["order"][start[l]:start[l + 1]].tolist()
            assert [lid[k] for k in words] == [l] * len(words) and [got["line_pos"][k] for k in words] == list(range(len(words))), name
            seen, todo = {words[0]}, [words[0]]                                                 # connected under Link
            while todo:
                i = todo.pop()
                for j in words:
                    if j not in seen and (i, j) in link:
                        seen.add(j); todo.append(j)
            assert seen == set(words), (name, l)
            if not valid[words[0]]:
                continue
            cx, cy, w, h, a = (float(v) for v in got["line_boxes"][l])                          # every member corner inside
            t = math.radians(a)
            U, V = (math.cos(t), -math.sin(t)), (math.sin(t), math.cos(t))
            slack = 1e-6 + 4 * float(np.spacing(np.float32(max(abs(cx), abs(cy), w, h))))       # (the box is rounded to float32)
            for k in words:
                (u, v), r = C._dirs(rows[k]), rows[k]
                for su in (0.5, -0.5):
                    for sv in (0.5, -0.5):
                        px, py = r[0] + su * r[2] * u[0] + sv * r[3] * v[0] - cx, r[1] + su * r[2] * u[1] + sv * r[3] * v[1] - cy
                        assert abs(px * U[0] + py * U[1]) <= w / 2 + slack and abs(px * V[0] + py * V[1]) <= h / 2 + slack, (name, l, k)


def test_value_errors():
    from glass_amd.postprocess.line_grouping import check_line_params, group_lines_host
    boxes = C.bridge()
    nan, inf = float("nan"), float("inf")
    for key in C.DEFAULTS:
        for bad in (nan, inf, -inf, -0.5, "wide", None):
            with pytest.raises(ValueError, match=key):
                group_lines_host(boxes, {key: bad})
            with pytest.raises(ValueError, match=key):
                check_line_params(**{key: bad})
    for key, bad in (("min_height_ratio", 1.0001), ("max_angle_diff", 180.5)):
        with pytest.raises(ValueError, match=key):
            group_lines_host(boxes, {key: bad})
    for good in ({"min_height_ratio": 1.0}, {"max_angle_diff": 180}, {"max_angle_diff": 0}, {"max_gap": 0, "max_offset": 0}, {}):
        group_lines_host(boxes, good)
    with pytest.raises(ValueError, match="1025 words"):
        group_lines_host(np.zeros((1025, 5), dtype=np.float32))
    with pytest.raises(TypeError):
        group_lines_host(boxes, {"max_slant": 1.0})
    assert check_line_params() == C.DEFAULTS
    # thresholds change the grouping: a gap of 15 px between words 20 px high
    assert group_lines_host(boxes, {"max_gap": 0.5})["line_count"] == 3
    assert group_lines_host(boxes, {"max_gap": 0.8})["line_count"] == 1
    # the binding refuses before it looks at the device
    from glass_amd.ops import native as K
    import torch
    b, c = torch.zeros((1, 4, 5)), torch.zeros((1,), dtype=torch.int32)
    for key in C.DEFAULTS:
        with pytest.raises(ValueError, match=key):
            K.group_lines(b, c, **{key: nan})
    with pytest.raises(ValueError, match="K <= 1024"):
        K.group_lines(torch.zeros((1, 1025, 5)), c)
    with pytest.raises(ValueError, match="K <= 1024"):
        K.group_lines(torch.zeros((4, 5)), c)


def test_feature_header_and_binding():
    import re
    from glass_amd import _lib
    from glass_amd.ops import native as K
    from glass_amd.postprocess import line_grouping
    with open(os.path.join(ROOT, "include", "glass_hip_feature_lines.h")) as fh:
        text = fh.read()
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
        assert not any(r in name for r in RESERVED), name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_lines.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_group_lines" not in fh.read(), other
    assert not any(r in text for r in RESERVED)
    assert "glass_hip_feature_lines.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    for word in ("symmetric pair rule", "connected components", "NOT linked", "smallest-index word", "ties by index",
                 "rounded to float32 once", "two columns interleave", "bit-identical", "no float atomics", "never read",
                 "copied bit for bit"):
        assert word in text, word                                      # the contract is stated where the entry points are declared
    assert int(re.search(r"#define GLASS_GROUP_LINES_MAX_K (\d+)", text).group(1)) == K.GROUP_LINES_MAX_K == line_grouping.MAX_WORDS
    assert K.GROUP_LINES_MAX_K == K.POSTPROCESS_MAX_K
    assert _lib.ABI_VERSION == 8


def test_config_keys_and_reference_yaml():
    from glass_amd.config import get_glass_cfg
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"))
    pp = cfg.POST_PROCESSING
    assert pp.GROUP_LINES is False
    assert (pp.LINE_MAX_ANGLE_DIFF, pp.LINE_MIN_HEIGHT_RATIO, pp.LINE_MAX_OFFSET, pp.LINE_MAX_GAP) == (15.0, 0.5, 0.5, 1.0)
    with open(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")) as fh:
        assert "GROUP_LINES" not in fh.read()                          # a file with the reference's keys only still loads
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    on = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.LINE_MAX_GAP", 2.0])
    assert on.POST_PROCESSING.GROUP_LINES is True and on.POST_PROCESSING.LINE_MAX_GAP == 2.0
    from glass_amd.postprocess import build_post_processor
    assert build_post_processor(cfg).line_params is None
    assert build_post_processor(on).line_params == dict(C.DEFAULTS, max_gap=2.0)
    bad = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.LINE_MIN_HEIGHT_RATIO", 1.5])
    with pytest.raises(ValueError, match="min_height_ratio"):
        build_post_processor(bad)
    off = get_glass_cfg(path, ["POST_PROCESSING.LINE_MIN_HEIGHT_RATIO", 1.5])       # unused while the key is off
    assert build_post_processor(off).line_params is None


def test_lines_of_on_hand_made_instances():
    import torch
    from glass_amd.postprocess import group_lines_host, lines_of
    from glass_amd.structures.core import Instances, RotatedBoxes
    boxes = C.opposite_lines()
    g = group_lines_host(boxes)
    inst = Instances((200, 500))
    inst.pred_boxes = RotatedBoxes(torch.from_numpy(boxes))
    with pytest.raises(ValueError, match="GROUP_LINES"):
        lines_of(inst)
    inst.pred_line_ids = torch.from_numpy(g["line_id"]).long()
    inst.pred_line_pos = torch.from_numpy(g["line_pos"]).long()
    inst.pred_line_boxes = torch.from_numpy(g["line_boxes"][g["line_id"]])
    lines = lines_of(inst)
    assert [ln["words"] for ln in lines] == [g["order"][a:b].tolist() for a, b in zip(g["line_start"][:-1], g["line_start"][1:])]
    assert all("text" not in ln for ln in lines) and lines[0]["box"] == [float(v) for v in g["line_boxes"][0]]
    inst.pred_texts = [f"w{k}" for k in range(len(boxes))]
    lines = lines_of(inst)
    assert [ln["text"] for ln in lines] == [" ".join(f"w{k}" for k in ln["words"]) for ln in lines]
    keep = torch.from_numpy(g["line_id"] == 1)                          # filtering keeps the fields in step
    sub = inst[keep]
    lines = lines_of(sub)
    assert len(lines) == 1 and sorted(lines[0]["words"]) == list(range(int(keep.sum())))
    assert lines[0]["text"] == " ".join(f"w{k}" for k in g["order"][g["line_start"][1]:g["line_start"][2]])
