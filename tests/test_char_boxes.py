"""Host: the statement of the character spans (glass_amd.postprocess.char_boxes.char_spans_host) against the independent exact
checker of char_box_cases.py on every case, known answers, the header and the bindings, the config key, and every ValueError /
NotImplementedError the feature raises before it looks at a device."""
import os
import re

import numpy as np
import pytest

import char_box_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "glass_hip_feature_chars.h"
NAMES = ["glass_forced_attention_workspace_bytes", "glass_forced_attention", "glass_char_spans", "glass_char_quads"]
KEY = "MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES"


def test_host_statement_equals_the_checker_on_every_case():
    from glass_amd.postprocess.char_boxes import char_spans_host
    cases = C.all_cases()
    seen = set()
    for name, att, tg, ln, ref in cases:
        got = char_spans_host(att, tg, ln, C.EOS)
        L = att.shape[1]
        worst = C.assert_matches_reference(got, ref, name, L)
        print(f"[chars] {name}: {att.shape[0]} words, L {L}, T {att.shape[2]}, counts {sorted(set(ref['count']))[:6]}, non-monotone "
              f"{ref['monotone'].count(0) - ref['valid'].count(0)}, invalid {ref['valid'].count(0)}, smallest centre gap "
              f"{ref['min_gap']:.2e}, worst float32 ulp {worst}")
        for r in range(att.shape[0]):                                  # everything from the count on is zero
            m = ref["count"][r]
            assert not got["spans"][r, m:].any() and not got["centres"][r, m:].any() and not got["spreads"][r, m:].any(), name
        seen.add(name)
    print(f"[chars] seeds tried {C.SEEDS_TRIED}, rejected {C.SEEDS_REJECTED}")
    assert C.SEEDS_TRIED == 20 and C.SEEDS_REJECTED <= 1
    assert {"T = 1", "T = 2", "T = 63", "T = 64", "m = 0, 1, 2, L"} <= seen
    # the seeded cases hold words of both kinds, so the flag is exercised
    mono = [v for n, *_, ref in cases if n.startswith("seed") for v, ok in zip(ref["monotone"], ref["valid"]) if ok]
    assert 0 in mono and 1 in mono


def test_known_answers():
    from glass_amd.postprocess.char_boxes import char_quads_host, char_spans_host
    by = {n: (a, t, ln, ref) for n, a, t, ln, ref in C.all_cases()}
    a, t, ln, _ = by["one-hot rows"]
    g = char_spans_host(a, t, ln, C.EOS)
    p = lambda j: (j + 0.5) / 16.0
    assert g["count"].tolist() == [4] and g["monotone"].tolist() == [1] and g["valid"].tolist() == [1]
    assert g["centres"][0, :4].tolist() == [p(1), p(4), p(9), p(15)] and not g["spreads"].any()     # exactly p_j, spread 0
    b = [(p(1) + p(4)) / 2, (p(4) + p(9)) / 2, (p(9) + p(15)) / 2]
    assert g["spans"][0, :4].tolist() == [[0.0, b[0]], [b[0], b[1]], [b[1], b[2]], [b[2], 1.0]]     # both edges clamped
    a, t, ln, _ = by["two equal peaks"]
    g = char_spans_host(a, t, ln, C.EOS)
    assert g["centres"][0, :2].tolist() == [p(4), p(10)] and g["spreads"][0, :2].tolist() == [2 / 16.0, 2 / 16.0]
    a, t, ln, _ = by["a uniform row"]
    g = char_spans_host(a, t, ln, C.EOS)
    assert g["centres"][0, :3].tolist() == [0.5] * 3 and g["monotone"].tolist() == [0]
    assert np.allclose(g["spreads"][0, :3], np.sqrt((16 * 16 - 1) / 12.0) / 16.0, rtol=1e-6, atol=0)
    a, t, ln, _ = by["a non-monotone word"]
    g = char_spans_host(a, t, ln, C.EOS)
    assert g["monotone"].tolist() == [0] and g["count"].tolist() == [4]
    assert (g["spans"][0, :4, 0] <= g["spans"][0, :4, 1]).all()        # the spans are defined by the rule all the same
    a, t, ln, _ = by["two steps with the same centre"]
    g = char_spans_host(a, t, ln, C.EOS)
    assert g["monotone"].tolist() == [0, 0]
    assert g["spans"][1, :2].tolist() == [[p(7), p(7)], [p(7), p(7)]]   # at the word's edge the mirrored span has zero width
    assert g["spans"][0, 1].tolist() == [(p(3) + p(7)) / 2, p(7)] and g["spans"][0, 2].tolist() == [p(7), (p(7) + p(12)) / 2]
    assert g["spans"][0, 1, 1] == g["spans"][0, 2, 0] == g["centres"][0, 1]     # the boundary between them is their centre:
    # step 1 ends and step 2 begins there; inside a word a zero-width span needs three equal centres
    three = C._batch([C._word(C._onehot(16, [3, 7, 7, 7, 12]), 8)])
    g3 = char_spans_host(*three, C.EOS)
    assert g3["spans"][0, 2].tolist() == [p(7), p(7)] and g3["monotone"].tolist() == [0]
    a, t, ln, _ = by["m = 0, 1, 2, L"]
    g = char_spans_host(a, t, ln, C.EOS)
    assert g["count"].tolist() == [0, 1, 2, 8] and g["monotone"].tolist() == [1, 1, 1, 1] and g["valid"].tolist() == [1, 1, 1, 1]
    assert g["spans"][1, 0].tolist() == [0.0, 1.0] and not g["spans"][0].any()
    a, t, ln, _ = by["a word without a stop symbol"]
    assert char_spans_host(a, t, ln, C.EOS)["count"].tolist() == [3] and ln.tolist() == [3]
    a, t, ln, _ = by["the stop at step 0"]
    assert char_spans_host(a, t, ln, C.EOS)["count"].tolist() == [0, 2] and ln.tolist() == [1, 3]
    a, t, ln, _ = by["lengths outside 0..L"]
    assert char_spans_host(a, t, ln, C.EOS)["count"].tolist() == [0, 8]
    a, t, ln, _ = by["a NaN, a negative, an infinite and an all-zero row"]
    g = char_spans_host(a, t, ln, C.EOS)
    assert g["valid"].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1] and g["count"].tolist() == [2, 0, 2, 0, 2, 0, 2, 0, 2]
    for r in (1, 3, 5, 7):                                             # an invalid word is all zero, its neighbours untouched
        assert not g["spans"][r].any() and not g["centres"][r].any() and g["monotone"][r] == 0
        assert g["centres"][r - 1, :2].tolist() == [p(1 + r // 2), p(9)] and g["centres"][r + 1, 0] > 0
    # a symbol is compared, never used as an index
    wild = by["one-hot rows"][1].copy()
    wild[0, :4] = [-7, 1 << 30, -(1 << 31), 999]
    assert char_spans_host(by["one-hot rows"][0], wild, by["one-hot rows"][2], C.EOS)["count"].tolist() == [4]
    # quads: a span (0, 1) is the word's own polygon, in the order of boxes_to_polygons
    import torch
    from glass_amd.postprocess.post_processor_rotated_boxes import PostProcessorRotatedBoxes
    frames = np.array([[50, 40, 30, 10, 0], [50, 40, 30, 10, 90], [20, 30, 8, 4, 30], [20, 30, 8, 4, -170]], dtype=np.float32)
    spans = np.zeros((4, 2, 2), dtype=np.float32); spans[:, 0] = [0.0, 1.0]; spans[:, 1] = [0.25, 0.5]
    q = char_quads_host(spans, np.array([2, 2, 1, 2]), frames)
    poly = PostProcessorRotatedBoxes.boxes_to_polygons(torch.from_numpy(frames).double()).numpy()
    assert np.abs(q[:, 0].astype(np.float64) - poly).max() < 1e-5
    assert q[0, 0].tolist() == [[35, 35], [65, 35], [65, 45], [35, 45]] and q[0, 1].tolist() == [[42.5, 35], [50, 35], [50, 45], [42.5, 45]]
    assert np.abs(q[1, 1] - np.array([[45, 47.5], [45, 40], [55, 40], [55, 47.5]])).max() < 1e-5      # 90 degrees: the width runs up
    assert not q[2, 1].any()                                           # from the count on


def test_feature_header_and_binding():
    import ctypes
    from glass_amd import _lib
    from glass_amd.ops import native as K
    from glass_amd.postprocess import char_boxes
    with open(os.path.join(ROOT, "include", HEADER)) as fh:
        text = fh.read()
    sigs = _lib.signatures(text)
    assert list(sigs) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):   # the names only in their own header
        if other != HEADER:
            with open(os.path.join(ROOT, "include", other)) as fh:
                body = fh.read()
            for name in ("glass_forced_attention", "glass_char_spans", "glass_char_quads"):
                assert name not in body, (other, name)
    assert HEADER in [os.path.basename(p) for p in _lib.feature_headers()]
    assert '#include "glass_hip.h"' in text
    words = " ".join(text.replace(" *", " ").split())
    for word in ("Row 0 comes from the step -1 launch", "row t + 1 comes from the launch of step t", "effective length", "bit for bit",
                 "keeps the rows it computed", "max_len + 1 launches", "no host synchronisation", "bit-identical from run to run",
                 "never used as an index", "widened exactly to float64", "rounded to float32 once", "the WORD is invalid",
                 "mirrored and clamped", "strictly increasing", "need not be monotone", "without contraction",
                 "R == 0 returns without one", "(cos t, -sin t)", "boxes_to_polygons", "gives zero rows"):
        assert word in words, word                                     # the contract is stated where the entry points are declared
    # restype and argtypes come from the header
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert sigs["glass_forced_attention_workspace_bytes"] == (i64, [i] * 6)
    assert sigs["glass_forced_attention"] == (i, [p, p, p] + [i] * 7 + [p] * 9 + [i64, p])
    assert sigs["glass_char_spans"] == (i, [p, p, p, i, i, i, i] + [p] * 7)
    assert sigs["glass_char_quads"] == (i, [p, p, p, i, i, p, p])
    # glass_forced_attention = the arguments of glass_forced_decode plus out_attention, before the workspace
    fd = _lib.signatures()["glass_forced_decode"]
    assert sigs["glass_forced_attention"][1] == fd[1][:17] + [p] + fd[1][17:]
    assert _lib.ABI_VERSION == 8
    _lib.build_library()
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == sigs[name], name
    for args in ((3, 5, 32, 256, 97, 26), (0, 5, 32, 256, 97, 26), (17, 16, 64, 256, 256, 64)):
        assert L.glass_forced_attention_workspace_bytes(*args) == L.glass_forced_decode_workspace_bytes(*args)
    assert K.CHAR_SPANS_MAX_STEPS == char_boxes.MAX_STEPS == 64 and K.CHAR_SPANS_MAX_COLUMNS == char_boxes.MAX_COLUMNS == 64
    # the library refuses bad sizes and null pointers before any launch (no device is touched)
    assert L.glass_char_spans(None, None, None, 0, 26, 32, 1, None, None, None, None, None, None, None) == 0
    assert L.glass_char_quads(None, None, None, 0, 26, None, None) == 0
    for bad in ((1, 0, 32), (1, 65, 32), (1, 26, 0), (1, 26, 65), (-1, 26, 32)):
        assert L.glass_char_spans(None, None, None, bad[0], bad[1], bad[2], 1, None, None, None, None, None, None, None) < 0
        assert b"glass_char_spans" in L.glass_last_error()
    assert L.glass_char_spans(None, None, None, 1, 26, 32, 1, None, None, None, None, None, None, None) < 0
    assert b"null pointer" in L.glass_last_error()
    assert L.glass_char_quads(None, None, None, 1, 65, None, None) < 0 and L.glass_char_quads(None, None, None, 2, 26, None, None) < 0
    assert L.glass_forced_attention(None, None, None, 0, 1, 32, 256, 97, 26, 0, *([None] * 9), 0, None) == 0
    assert L.glass_forced_attention(None, None, None, 2, 17, 8, 256, 13, 5, 0, *([None] * 9), 0, None) < 0
    assert L.glass_last_error().decode().startswith("glass_forced_attention: needs D=256, 1<=T<=64")


def test_config_key_and_reference_yaml():
    from glass_amd.config import get_glass_cfg
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    assert get_glass_cfg().MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES is False
    cfg = get_glass_cfg(path)
    assert cfg.MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES is False
    for name in sorted(os.listdir(os.path.join(ROOT, "configs"))):
        with open(os.path.join(ROOT, "configs", name)) as fh:
            assert "CHAR_BOXES" not in fh.read(), name                 # a file with the reference's keys only still loads
    assert get_glass_cfg(path, [KEY, True]).MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES is True
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert "CHAR_BOXES" in fh.read()
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3, split_text_rows
    from glass_amd.structures.core import ShapeSpec
    assert RecognizerRCNNHeadV3(cfg, ShapeSpec(channels=256)).char_boxes is False
    for opts in ([], ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 5], ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 5,
                                                                   "MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS", True]):
        assert RecognizerRCNNHeadV3(get_glass_cfg(path, [KEY, True] + opts), ShapeSpec(channels=256)).char_boxes is True
    # existing callers of split_text_rows keep their pair; the third member is asked for
    assert split_text_rows("rows") == ("rows", None) and split_text_rows(("rows", "dist")) == ("rows", "dist")
    assert split_text_rows(("rows", None, "chars")) == ("rows", None)
    assert split_text_rows("rows", chars=True) == ("rows", None, None)
    assert split_text_rows(("rows", "dist"), chars=True) == ("rows", "dist", None)
    assert split_text_rows(("rows", None, "chars"), chars=True) == ("rows", None, "chars")


def test_errors_raised_before_any_device_work():
    import torch
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_decoder import ForcedResult
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.ops import native as K
    from glass_amd.postprocess import char_quads, char_spans_host, chars_of
    from glass_amd.structures.core import Instances, RotatedBoxes, ShapeSpec
    att, tg, ln = torch.zeros((2, 26, 32)), torch.zeros((2, 26), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    for bad in (torch.zeros((2, 65, 32)), torch.zeros((2, 26, 65)), torch.zeros((2, 0, 32)), torch.zeros((26, 32)), None):
        with pytest.raises(ValueError, match="attention"):
            K.char_spans(bad, tg, ln, 1)
    with pytest.raises(ValueError, match="targets"):
        K.char_spans(att, tg[:1], ln, 1)
    with pytest.raises(ValueError, match="lengths"):
        K.char_spans(att, tg, ln[:1], 1)
    with pytest.raises(ValueError, match="spans"):
        K.char_quads(torch.zeros((2, 26, 3)), ln, torch.zeros((2, 5)))
    with pytest.raises(ValueError, match="count"):
        K.char_quads(torch.zeros((2, 26, 2)), ln[:1], torch.zeros((2, 5)))
    with pytest.raises(ValueError, match="frames"):
        K.char_quads(torch.zeros((2, 26, 2)), ln, torch.zeros((2, 4)))
    from glass_amd import _lib
    with pytest.raises(_lib.GlassLibraryError):                        # no CPU fallback
        K.char_spans(att, tg, ln, 1)
    with pytest.raises(_lib.GlassLibraryError):
        K.char_quads(torch.zeros((2, 26, 2)), ln, torch.zeros((2, 5)))
    x = torch.zeros((1, 4, 256))
    with pytest.raises(_lib.GlassLibraryError):
        K.forced_decode(x, x, {}, torch.zeros((1, 1, 26), dtype=torch.int32), None, 97, 26, 0, attention=True)
    for bad in (np.zeros((2, 65, 4)), np.zeros((2, 4, 65)), np.zeros((4, 4))):
        with pytest.raises(ValueError, match="attention"):
            char_spans_host(bad, np.zeros((2, 4)), np.zeros((2,)), 1)
    with pytest.raises(ValueError, match="targets"):
        char_spans_host(np.zeros((2, 4, 4)), np.zeros((2, 5)), np.zeros((2,)), 1)
    # instances without the fields name the key
    inst = Instances((10, 10))
    inst.pred_boxes = RotatedBoxes(torch.zeros((0, 5)))
    with pytest.raises(ValueError, match="CHAR_BOXES"):
        char_quads(inst)
    with pytest.raises(ValueError, match="CHAR_BOXES"):
        chars_of(inst, None)
    # the list-wise surface of the head raises, naming the key
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    head = RecognizerRCNNHeadV3(get_glass_cfg(path, [KEY, True]), ShapeSpec(channels=256))
    with pytest.raises(NotImplementedError, match="CHAR_BOXES"):
        head.forward(torch.zeros((1, 256, 8, 32)), [inst])
    # ForcedResult keeps its tuple length; the rows ride as an attribute
    r = ForcedResult(1, 2, 3, 4, 5, attention=6)
    a, b, c, d, e = r
    assert (a, b, c, d, e) == (1, 2, 3, 4, 5) and len(r) == 5 and r.attention == 6 and r.logits == 5
    assert ForcedResult(1, 2, 3, None, None).attention is None and ForcedResult._fields == ("step_logp", "scores", "lengths", "probs", "logits")


def test_packed_rows_and_fields_survive_indexing():
    import torch
    from glass_amd.postprocess.char_boxes import CHAR_FIELDS, attach_chars, char_spans_host, pack_chars, unpack_chars
    from glass_amd.structures.core import Instances, RotatedBoxes
    name, att, tg, ln, ref = [c for c in C.all_cases() if c[0] == "seed 4"][0]
    host = char_spans_host(att, tg, ln, C.EOS)
    packed = pack_chars({k: torch.from_numpy(v) for k, v in host.items()})
    R, L = att.shape[:2]
    assert packed.shape == (R, L + 1, 3) and packed.dtype == torch.float32
    f = unpack_chars(packed)
    assert torch.equal(f["pred_char_spans"], torch.from_numpy(host["spans"])) and torch.equal(f["pred_char_centres"], torch.from_numpy(host["centres"]))
    assert f["pred_char_count"].dtype == torch.int64 and f["pred_char_count"].tolist() == host["count"].tolist()
    assert f["pred_char_monotone"].dtype == torch.bool and f["pred_char_monotone"].tolist() == [bool(v) for v in host["monotone"]]
    inst = Instances((100, 200))
    boxes = torch.arange(R * 5, dtype=torch.float32).view(R, 5)
    inst.pred_boxes = RotatedBoxes(boxes.clone())
    attach_chars(inst, packed, inst.pred_boxes.tensor)
    assert all(inst.has(k) for k in CHAR_FIELDS)
    inst.pred_boxes.tensor[:, 2] += 50.0                               # the merge step may enlarge pred_boxes; the frame stays
    assert torch.equal(inst.pred_char_frames, boxes)
    keep = torch.arange(R) % 2 == 0
    sub = inst[keep]
    assert len(sub) == int(keep.sum()) and torch.equal(sub.pred_char_spans, f["pred_char_spans"][keep])
    assert torch.equal(sub.pred_char_count, f["pred_char_count"][keep]) and torch.equal(sub.pred_char_frames, boxes[keep])
    assert torch.equal(sub.pred_char_monotone, f["pred_char_monotone"][keep]) and torch.equal(inst[1].pred_char_centres, f["pred_char_centres"][1:2])
