"""Host: the statement of the page order (glass_amd.postprocess.line_order.order_lines_host) against the independent checker of
line_order_cases.py on every case, the order of construction on the page scenes, every ValueError, the header, the config
keys, and `blocks_of` / `page_text` on hand-made Instances."""
import os

import numpy as np
import pytest

import line_order_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glass_order_lines_workspace_bytes", "glass_order_lines"]
RESERVED = ("glass_ring_simplify", "glass_beam_search_merged", "glass_beam_search_dfa", "glass_beam_search_wdfa", "glass_roi_mask",
            "glass_group_lines")


def _assert_equal(got, ref, name):
    assert got["block_count"] == ref["block_count"] and got["forced"] == ref["forced"], name
    for k in C.INT_FIELDS:
        assert got[k].dtype == np.int32 and got[k].tolist() == ref[k], (name, k)
    assert got["block_boxes"].dtype == np.float32 and got["block_boxes"].shape == (ref["block_count"], 5), name
    for b in range(ref["block_count"]):
        assert C.box_ulps(got["block_boxes"][b], ref["block_boxes"][b]) <= 1, (name, b)


def test_equals_the_checker_on_every_case():
    from glass_amd.postprocess.line_order import order_lines_host
    forced = blocks = 0
    for name, boxes, built, ref in C.all_cases():
        got = order_lines_host(boxes)
        print(f"[line_order] {name}: {len(boxes)} lines, {ref['block_count']} blocks, {ref['edges']} edges, {ref['forced']} forced, "
              f"margins {ref['cmp_margin']:.2e} / {ref['key_margin']:.2e}")
        _assert_equal(got, ref, name)
        forced += ref["forced"] > 0
        blocks += ref["block_count"] not in (0, 1, len(boxes))
    assert forced >= 3 and blocks >= 8                                 # cycles happen, and the cuts are no trivial ones


def test_the_pages_read_in_the_order_they_were_built():
    for name in C.PAGES:
        _, boxes, built, ref = C.case(name)
        assert ref["page_order"] == built, name
        assert ref["forced"] == 0, name
        assert sorted(ref["page_order"]) == list(range(len(boxes))), name
    # a column page is not read top to bottom: the key order (what the line grouping's rank gives) interleaves the columns
    _, boxes, built, ref = C.case("3 columns")
    assert ref["page_order"] != sorted(range(len(boxes)), key=lambda k: (float(boxes[k, 1]), float(boxes[k, 0])))
    # paragraphs: three per column and the header
    assert C.case("2 columns")[3]["block_count"] == 1 + 2 * 3 and C.case("4 columns")[3]["block_count"] == 1 + 4 * 3


def test_known_answers():
    from glass_amd.postprocess.line_order import order_lines_host
    boxes = C.four_line_cycle()[0]
    ref = C.reference(boxes)
    assert ref["page_order"] == [2, 3, 0, 1] and ref["forced"] == 1 and ref["cmp_margin"] >= 1.0
    got = order_lines_host(boxes)
    assert got["page_order"].tolist() == [2, 3, 0, 1] and got["forced"] == 1 and got["page_rank"].tolist() == [2, 3, 0, 1]
    assert C.case("random overlapping boxes")[3]["forced"] > 0 and C.case("random overlapping boxes, 65")[3]["forced"] > 0
    got = order_lines_host(C.identical(70)[0])                          # all ties: no edge, the index decides, no two share a block
    assert got["page_order"].tolist() == list(range(70)) and got["block_count"] == 70 and got["forced"] == 0
    empty = order_lines_host(np.zeros((0, 5), dtype=np.float32))
    assert empty["block_count"] == 0 and empty["block_start"].tolist() == [0] and empty["block_boxes"].shape == (0, 5)
    one = order_lines_host(np.array([[10, 20, 30, 8, 0]], dtype=np.float32))
    assert one["page_order"].tolist() == [0] and one["block_boxes"].tolist() == [[10.0, 20.0, 30.0, 8.0, 0.0]]
    # an invalid line is a block of its own, after the valid ones, its box its own values bit for bit
    name, boxes, built, ref = C.case("lines that are no lines")
    got = order_lines_host(boxes)
    bad = [k for k in range(len(boxes)) if not ref["valid"][k]]
    assert len(bad) == 9 and got["page_order"][-9:].tolist() == bad
    for k in bad:
        assert got["block_boxes"][got["block_id"][k]].view(np.uint32).tolist() == boxes[k].view(np.uint32).tolist()
    # two stacked lines: one block while the gap allows it
    two = np.array([[100, 100, 200, 20, 0], [100, 130, 200, 20, 0]], dtype=np.float32)      # a gap of 10 px = 0.5 h
    assert order_lines_host(two)["block_count"] == 1
    assert order_lines_host(two, {"block_max_gap": 0.4})["block_count"] == 2
    two[1, 3] = 12.0                                                   # 12 / 20 = 0.6 of the taller
    assert order_lines_host(two)["block_count"] == 2
    assert order_lines_host(two, {"block_min_height_ratio": 0.5})["block_count"] == 1
    side = np.array([[300, 100, 200, 20, 0], [120, 108, 200, 20, 0]], dtype=np.float32)     # 20 px of 200 shared: left one first
    assert order_lines_host(side, {"min_overlap": 0.2})["page_order"].tolist() == [1, 0]
    assert order_lines_host(side, {"min_overlap": 0.05})["page_order"].tolist() == [0, 1]


def test_line_first_counts_the_words_ahead():
    from glass_amd.postprocess.line_order import order_lines_host
    name, boxes, built, ref = C.case("3 columns")
    L = len(boxes)
    rng = np.random.RandomState(3)
    start = np.concatenate([[0], np.cumsum(rng.randint(1, 6, size=L))]).astype(np.int32)
    K = int(start[-1])                                                 # K words in L lines: the CSR has K + 1 entries
    start = np.concatenate([start, np.full((K - L,), K, dtype=np.int32)])
    got = order_lines_host(boxes, line_start=start, K=K)
    assert got["line_first"].dtype == np.int32 and got["line_first"].tolist() == C.line_first(ref, start, K)
    sizes = np.diff(start)
    assert got["line_first"][got["page_order"]].tolist() == np.concatenate([[0], np.cumsum(sizes[got["page_order"]])[:-1]]).tolist()
    hostile = start.copy()
    hostile[5], hostile[17], hostile[40] = -4, K + 9, 0
    got = order_lines_host(boxes, line_start=hostile, K=K)
    assert got["line_first"].tolist() == C.line_first(ref, hostile, K)
    assert "line_first" not in order_lines_host(boxes)
    with pytest.raises(ValueError, match="line_start"):
        order_lines_host(boxes, line_start=start[:L])


def test_value_errors():
    from glass_amd.postprocess.line_order import check_order_params, order_lines_host
    boxes = C.four_line_cycle()[0]
    nan, inf = float("nan"), float("inf")
    for key in C.DEFAULTS:
        for bad in (nan, inf, -inf, -0.5, "wide", None, True):
            with pytest.raises(ValueError, match=key):
                order_lines_host(boxes, {key: bad})
            with pytest.raises(ValueError, match=key):
                check_order_params(**{key: bad})
    for key, bad in (("min_overlap", 1.0), ("min_overlap", 1.5), ("block_min_height_ratio", 1.0001)):
        with pytest.raises(ValueError, match=key):
            order_lines_host(boxes, {key: bad})
    for good in ({"min_overlap": 0}, {"min_overlap": 0.999}, {"block_min_height_ratio": 1.0}, {"block_min_height_ratio": 0},
                 {"block_max_gap": 0}, {"block_max_gap": 1e6}, {}):
        order_lines_host(boxes, good)
    with pytest.raises(ValueError, match="1025 lines"):
        order_lines_host(np.zeros((1025, 5), dtype=np.float32))
    with pytest.raises(TypeError):
        order_lines_host(boxes, {"max_slant": 1.0})
    assert check_order_params() == C.DEFAULTS
    # the binding refuses before it looks at the device
    from glass_amd.ops import native as K
    import torch
    b, c = torch.zeros((1, 4, 5)), torch.zeros((1,), dtype=torch.int32)
    for key in C.DEFAULTS:
        with pytest.raises(ValueError, match=key):
            K.order_lines(b, c, **{key: nan})
    with pytest.raises(ValueError, match="K <= 1024"):
        K.order_lines(torch.zeros((1, 1025, 5)), c)
    with pytest.raises(ValueError, match="K <= 1024"):
        K.order_lines(torch.zeros((4, 5)), c)
    with pytest.raises(ValueError, match="line_count"):
        K.order_lines(b, torch.zeros((2,), dtype=torch.int32))
    with pytest.raises(ValueError, match="line_start"):
        K.order_lines(b, c, torch.zeros((1, 4), dtype=torch.int32))


def test_feature_header_and_binding():
    import re
    from glass_amd import _lib
    from glass_amd.ops import native as K
    from glass_amd.postprocess import line_order
    with open(os.path.join(ROOT, "include", "glass_hip_feature_layout.h")) as fh:
        text = fh.read()
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
        assert not any(r in name for r in RESERVED), name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_layout.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_order_lines" not in fh.read(), other
    assert not any(r in text for r in RESERVED)
    assert "glass_hip_feature_layout.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    for word in ("Rule 1", "Rule 2", "symmetric", "fixed-shape tree sum", "smallest key", "forced", "in index order", "maximal runs",
                 "a negative gap passes", "rounded to float32 once", "copied bit for bit", "never read", "no float atomics",
                 "without contraction", "bit-identical", "does not depend on its neighbours", "used as an index unchecked",
                 "runs exactly L times", "a table", "L-shaped", "line_first[line] + line_pos"):
        assert word in " ".join(text.replace(" *", " ").split()), word   # the contract is stated where the entry points are declared
    assert int(re.search(r"#define GLASS_ORDER_LINES_MAX_K (\d+)", text).group(1)) == K.ORDER_LINES_MAX_K == line_order.MAX_LINES
    assert K.ORDER_LINES_MAX_K == K.GROUP_LINES_MAX_K
    assert _lib.ABI_VERSION == 8
    # the three places that state the limit of the line grouping keep their words and point here
    for path in ("include/glass_hip_feature_lines.h", "glass-text-spotting_amd/glass_amd/postprocess/line_grouping.py", "README.md"):
        with open(os.path.join(ROOT, path)) as fh:
            words = " ".join(fh.read().replace(" *", " ").split())
        assert "two columns interleave" in words and "ORDER_LINES" in words, path


def test_config_keys_and_reference_yaml():
    from glass_amd.config import get_glass_cfg
    from glass_amd.postprocess import build_post_processor
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    cfg = get_glass_cfg(path)
    pp = cfg.POST_PROCESSING
    assert pp.ORDER_LINES is False
    assert (pp.ORDER_MIN_OVERLAP, pp.BLOCK_MAX_GAP, pp.BLOCK_MIN_HEIGHT_RATIO) == (0.1, 0.8, 0.7)
    with open(path) as fh:
        assert "ORDER_LINES" not in fh.read()                          # a file with the reference's keys only still loads
    assert build_post_processor(cfg).order_params is None
    lines_only = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True])
    assert build_post_processor(lines_only).order_params is None
    on = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ORDER_LINES", True, "POST_PROCESSING.BLOCK_MAX_GAP", 1.5])
    assert on.POST_PROCESSING.ORDER_LINES is True
    assert build_post_processor(on).order_params == dict(C.DEFAULTS, block_max_gap=1.5)
    with pytest.raises(ValueError, match="GROUP_LINES"):
        build_post_processor(get_glass_cfg(path, ["POST_PROCESSING.ORDER_LINES", True]))
    for key, name, bad in (("ORDER_MIN_OVERLAP", "min_overlap", 1.0), ("BLOCK_MAX_GAP", "block_max_gap", -1.0),
                           ("BLOCK_MIN_HEIGHT_RATIO", "block_min_height_ratio", 1.5)):
        opts = ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ORDER_LINES", True, f"POST_PROCESSING.{key}", bad]
        with pytest.raises(ValueError, match=name):
            build_post_processor(get_glass_cfg(path, opts))
        off = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, f"POST_PROCESSING.{key}", bad])   # unused while the key is off
        assert build_post_processor(off).order_params is None


def test_blocks_of_and_page_text_on_hand_made_instances():
    import torch
    from glass_amd.postprocess import blocks_of, group_lines_host, order_lines_host, page_text
    from glass_amd.structures.core import Instances, RotatedBoxes
    # two columns of two paragraphs of two lines of two words; the words are numbered in reading order, then shuffled
    rows = []
    for col in range(2):
        for para in range(2):
            for line in range(2):
                for word in range(2):
                    rows.append([100.0 + 400.0 * col + 70.0 * word, 100.0 + 160.0 * para + 30.0 * line + 2.0 * col, 60.0, 20.0, 0.0])
    perm = np.random.RandomState(0).permutation(len(rows))
    boxes = np.asarray(rows, dtype=np.float32)[perm]
    g = group_lines_host(boxes)
    assert g["line_count"] == 8
    p = order_lines_host(g["line_boxes"], line_start=g["line_start"])
    assert p["block_count"] == 4 and p["forced"] == 0
    inst = Instances((500, 900))
    inst.pred_boxes = RotatedBoxes(torch.from_numpy(boxes))
    inst.pred_line_ids = torch.from_numpy(g["line_id"]).long()
    inst.pred_line_pos = torch.from_numpy(g["line_pos"]).long()
    inst.pred_line_boxes = torch.from_numpy(g["line_boxes"][g["line_id"]])
    with pytest.raises(ValueError, match="ORDER_LINES"):
        blocks_of(inst)
    inst.pred_page_rank = torch.from_numpy(p["line_first"][g["line_id"]] + g["line_pos"]).long()
    inst.pred_block_ids = torch.from_numpy(p["block_id"][g["line_id"]]).long()
    inst.pred_block_boxes = torch.from_numpy(p["block_boxes"][p["block_id"][g["line_id"]]])
    assert inst.pred_page_rank[torch.from_numpy(np.argsort(perm))].tolist() == list(range(16))     # word k of the construction is k-th
    blocks = blocks_of(inst)
    assert [[[int(perm[k]) for k in ln["words"]] for ln in b["lines"]] for b in blocks] == \
        [[[8 * c + 4 * q, 8 * c + 4 * q + 1], [8 * c + 4 * q + 2, 8 * c + 4 * q + 3]] for c in range(2) for q in range(2)]
    assert all("text" not in ln for b in blocks for ln in b["lines"])
    assert blocks[0]["box"] == [float(v) for v in p["block_boxes"][0]] == [135.0, 115.0, 130.0, 50.0, 0.0]
    assert blocks[0]["lines"][1]["box"] == [135.0, 130.0, 130.0, 20.0, 0.0]
    with pytest.raises(ValueError, match="pred_texts"):
        page_text(inst)
    inst.pred_texts = [f"w{int(perm[k])}" for k in range(16)]
    assert page_text(inst) == "w0 w1\nw2 w3\n\nw4 w5\nw6 w7\n\nw8 w9\nw10 w11\n\nw12 w13\nw14 w15"
    # the top-to-bottom rank of the line grouping interleaves the columns on the same page
    reading = np.empty((16,), dtype=np.int64)
    reading[g["order"]] = np.arange(16)
    assert [int(perm[k]) for k in np.argsort(reading)][:4] == [0, 1, 8, 9]
    keep = torch.from_numpy(np.isin(perm, (2, 3, 9, 12, 13, 14, 15)))   # filtering keeps the fields in step
    assert page_text(inst[keep]) == "w2 w3\n\nw9\n\nw12 w13\nw14 w15"
