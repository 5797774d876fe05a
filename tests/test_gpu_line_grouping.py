"""GPU: glass_group_lines (csrc/line_group.hip) through ops.native.group_lines against the independent checker of
line_group_cases.py - line_id, line_pos, order, line_start and line_count exactly, line_boxes within one float32 unit in the
last place of the checker's float64 box - at every size where the kernels take another path, on the hand-made scenes, with
padding rows of NaN and 1e30; determinism; and the post-processor with POST_PROCESSING.GROUP_LINES through run_batch,
run_tiled and __call__."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import line_group_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_FIELDS = ("line_id", "line_pos", "order", "line_start")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _batch(images, K):
    """boxes float32 [N, K, 5] with the images' words first and NaN / 1e30 rows beyond, counts int32 [N]"""
    boxes = np.empty((len(images), K, 5), dtype=np.float32)
    boxes[:, 0::2], boxes[:, 1::2] = np.nan, 1e30
    for n, b in enumerate(images):
        boxes[n, :len(b)] = b
    return boxes, np.array([len(b) for b in images], dtype=np.int32)


def _run(boxes, counts, **params):
    from glass_amd.ops import native as K
    out = K.group_lines(torch.from_numpy(boxes).to(_dev()), torch.from_numpy(counts).to(_dev()), **params)
    assert sorted(out) == sorted(INT_FIELDS + ("line_boxes", "line_count"))
    N, Kk = boxes.shape[:2]
    shapes = {"line_id": (N, Kk), "line_pos": (N, Kk), "order": (N, Kk), "line_start": (N, Kk + 1), "line_boxes": (N, Kk, 5),
              "line_count": (N,)}
    for k, v in out.items():
        assert tuple(v.shape) == shapes[k] and v.dtype == (torch.float32 if k == "line_boxes" else torch.int32), k
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(out, n, ref, K, what):
    want = C.expected_padded(ref, K)
    assert int(out["line_count"][n]) == want["line_count"], what
    for k in INT_FIELDS:
        got = out[k][n].tolist()
        assert got == want[k], f"{what}, {k}: first difference at {next(i for i, (a, b) in enumerate(zip(got, want[k])) if a != b)}"
    L = ref["line_count"]
    worst = max([C.box_ulps(out["line_boxes"][n, l], ref["line_boxes"][l]) for l in range(L)], default=0)
    assert worst <= 1, f"{what}: a line box {worst} float32 ulps from the checker's"
    assert not out["line_boxes"][n, L:].view(np.uint32).any(), what           # zeros beyond the line count
    return worst


@pytest.mark.parametrize("K", C.K_LIST)
def test_sizes_with_counts_0_K_and_half(K):
    full, half = C.case(f"paragraph of {K}" if K else "no words"), C.case(f"paragraph of {K // 2}" if K // 2 else "no words")
    boxes, counts = _batch([np.zeros((0, 5), dtype=np.float32), full[1], half[1]], K)
    assert counts.tolist() == [0, K, K // 2]
    out = _run(boxes, counts)
    _check(out, 0, C.case("no words")[2], K, f"K={K}, no words")
    _check(out, 1, full[2], K, f"K={K}, {K} words")
    _check(out, 2, half[2], K, f"K={K}, {K // 2} words")


def test_the_large_scenes():
    names = ("one line of 1024", "1024 singletons", "paragraph at 30 degrees", "paragraph at -170 degrees")
    cases = [C.case(n) for n in names]
    out = _run(*_batch([c[1] for c in cases], 1024))
    for n, (name, _, ref) in enumerate(cases):
        print(f"[line_group] {name}: {ref['line_count']} lines, worst box {_check(out, n, ref, 1024, name)} ulp")
    assert out["line_count"].tolist() == [1, 1024, cases[2][2]["line_count"], cases[3][2]["line_count"]]


def test_the_hand_made_scenes():
    names = ("opposite lines", "bridge", "arc of 120 degrees", "closed circle", "identical boxes", "words that are no words")
    cases = [C.case(n) for n in names]
    out = _run(*_batch([c[1] for c in cases], 70))
    for n, (name, _, ref) in enumerate(cases):
        _check(out, n, ref, 70, name)
    assert out["line_count"].tolist()[:5] == [2, 1, 1, 1, 1]
    boxes, ref = cases[5][1], cases[5][2]
    for k in range(len(boxes)):                                        # an invalid word's line box: its own bits
        if not ref["valid"][k]:
            assert out["line_boxes"][5, out["line_id"][5, k]].view(np.uint32).tolist() == boxes[k].view(np.uint32).tolist()


def test_counts_are_clamped_and_thresholds_reach_the_kernel():
    name, b, ref = C.case("paragraph of 64")
    boxes, counts = _batch([b, b, b], 64)
    out = _run(boxes, np.array([64 + 7, -3, 64], dtype=np.int32))
    _check(out, 0, ref, 64, "count above K")
    _check(out, 1, C.case("no words")[2], 64, "negative count")
    _check(out, 2, ref, 64, "count = K")
    bridge = C.bridge()
    for params, lines in (({"max_gap": 0.5}, 3), ({"max_gap": 0.8}, 1), ({"max_angle_diff": 0.0, "max_offset": 0.0}, 1),
                          ({"min_height_ratio": 1.0}, 1)):
        out = _run(*_batch([bridge], 3), **params)
        _check(out, 0, C.reference(bridge, dict(C.DEFAULTS, **params)), 3, str(params))
        assert int(out["line_count"][0]) == lines, params
    from glass_amd.ops import native as K
    dev = _dev()
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        for bad in ({"max_gap": float("nan")}, {"max_offset": -1}, {"min_height_ratio": 1.5}, {"max_angle_diff": 181}):
            with pytest.raises(ValueError):
                K.group_lines(torch.zeros((1, 4, 5), device=dev), torch.zeros((1,), dtype=torch.int32, device=dev), **bad)
        with pytest.raises(ValueError, match="K <= 1024"):
            K.group_lines(torch.zeros((1, 1025, 5), device=dev), torch.zeros((1,), dtype=torch.int32, device=dev))
        out = K.group_lines(torch.zeros((0, 8, 5), device=dev), torch.zeros((0,), dtype=torch.int32, device=dev))
        assert tuple(out["line_start"].shape) == (0, 9)


def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_neighbours():
    cases = [C.case(n) for n in ("paragraph of 511", "paragraph at 30 degrees", "closed circle", "paragraph of 129")]
    boxes, counts = _batch([c[1] for c in cases], 600)
    a, b = _run(boxes, counts), _run(boxes, counts)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for n in (0, 2):                                                   # alone, and after other neighbours
        alone = _run(boxes[n:n + 1], counts[n:n + 1])
        moved = _run(boxes[[3, 1, n]], counts[[3, 1, n]])
        for k in a:
            assert np.array_equal(alone[k][0].view(np.uint32), a[k][n].view(np.uint32)), (k, n)
            assert np.array_equal(moved[k][2].view(np.uint32), a[k][n].view(np.uint32)), (k, n)


# ------------------------------------------------------------------------------------------------ the post-processor
RUNNER_OPTS = ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "POST_PROCESSING.TEXT_THRESHOLD", 0.0,
               "POST_PROCESSING.GROUP_LINES", True]
NEW_FIELDS = ("pred_line_ids", "pred_line_pos", "pred_reading_rank", "pred_line_boxes")


@pytest.fixture(scope="module")
def runner():
    from glass_amd.config import get_glass_cfg
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), RUNNER_OPTS)
    return GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)


def _assert_fields(inst, what):
    """the new fields of one Instances against the host statement and the checker on the boxes it returns"""
    from glass_amd.postprocess import group_lines_host, lines_of
    boxes = inst.pred_boxes.tensor.cpu().numpy()
    c = len(boxes)
    host, ref = group_lines_host(boxes), C.reference(boxes)
    for name in NEW_FIELDS:
        assert inst.has(name) and len(inst.get(name)) == c, (what, name)
    for name in NEW_FIELDS[:3]:
        assert inst.get(name).dtype == torch.int64, (what, name)
    assert inst.pred_line_ids.tolist() == host["line_id"].tolist() == ref["line_id"], what
    assert inst.pred_line_pos.tolist() == host["line_pos"].tolist(), what
    rank = np.empty((c,), dtype=np.int64)
    rank[host["order"]] = np.arange(c)
    assert inst.pred_reading_rank.tolist() == rank.tolist(), what
    got = inst.pred_line_boxes.cpu().numpy()
    assert got.shape == (c, 5) and got.dtype == np.float32, what
    for k in range(c):
        assert C.box_ulps(got[k], host["line_boxes"][host["line_id"][k]]) <= 1, (what, k)
    lines = lines_of(inst)
    assert [ln["words"] for ln in lines] == [ref["order"][a:b] for a, b in zip(ref["line_start"][:-1], ref["line_start"][1:])], what
    if inst.has("pred_texts"):
        assert [ln["text"] for ln in lines] == [" ".join(inst.pred_texts[k] for k in ln["words"]) for ln in lines], what
    return len(lines)


def _same_but_for_the_lines(on, off, what):
    assert len(on) == len(off) and on.image_size == off.image_size, what
    fields_on, fields_off = on.get_fields(), off.get_fields()
    assert sorted(fields_on) == sorted(list(fields_off) + list(NEW_FIELDS)), what
    for name, v in fields_off.items():
        w = fields_on[name]
        if isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and torch.equal(v.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), (what, name)
        elif hasattr(v, "tensor"):
            assert torch.equal(v.tensor.contiguous().view(torch.uint8), w.tensor.contiguous().view(torch.uint8)), (what, name)
        else:
            assert v == w, (what, name)


def test_run_batch_and_run_tiled_carry_the_lines_and_without_the_key_nothing_changes(runner):
    from glass_amd.ops import native as K
    from glass_amd.utils.synth import make_image
    pp = runner.post_processor
    assert pp.line_params == C.DEFAULTS
    imgs = [make_image(5, 100, 80).numpy(), make_image(9, 250, 180).numpy()]
    big = make_image(3, 160, 224).numpy()
    tiled = dict(tile=128, overlap=64, border=8)
    on = runner.run_batch(imgs) + [runner.run_tiled(big, **tiled)]
    words = 0
    for n, inst in enumerate(on):
        assert len(inst) > 0, n
        lines = _assert_fields(inst, f"image {n}")
        print(f"[line_group] image {n}: {len(inst)} words in {lines} lines")
        words += len(inst)
    assert words >= 3
    params, pp.line_params = pp.line_params, None                      # what the constructor leaves with the key off
    try:
        with mock.patch.object(K, "group_lines", side_effect=AssertionError("launched")):
            off = runner.run_batch(imgs) + [runner.run_tiled(big, **tiled)]
    finally:
        pp.line_params = params
    for n, (a, b) in enumerate(zip(on, off)):
        _same_but_for_the_lines(a, b, f"image {n}")


def test_the_padded_tensors_travel_with_the_step(runner):
    name, boxes, ref = C.case("paragraph of 63")
    dev = _dev()
    b, counts = _batch([boxes, boxes[:20]], 140)                       # K > 128: behind the dense word kernel
    b[~np.isfinite(b) | (b > 1e20)] = 0.0                              # (plain padding: the word kernel's is not this test's subject)
    scores = torch.full((2, 140), 0.9, device=dev)
    res = runner.post_processor.process_padded(torch.from_numpy(b).to(dev), scores, torch.from_numpy(counts).to(dev), None, None,
                                               [(1200, 1200), (1200, 1200)])
    w = res.words
    assert w["count"].tolist() == [63, 20] and tuple(w["order"].shape) == (2, 140) and tuple(w["line_start"].shape) == (2, 141)
    for n, inst in enumerate(res):
        _assert_fields(inst, f"padded {n}")
        c = len(inst)
        assert w["line_id"][n, :c].tolist() == inst.pred_line_ids.tolist() and w["line_id"][n, c:].tolist() == [-1] * (140 - c)
        assert inst.pred_reading_rank[w["order"][n, :c].long()].tolist() == list(range(c))
    assert res[0].pred_line_ids.tolist() == ref["line_id"]             # (no word of the paragraph is merged or dropped)


def test_call_on_one_instances(runner):
    from glass_amd.postprocess import lines_of
    from glass_amd.structures.core import Instances, RotatedBoxes
    name, boxes, ref = C.case("paragraph of 63")
    dev = _dev()
    inst = Instances((1200, 1200))
    inst.pred_boxes = RotatedBoxes(torch.from_numpy(boxes).to(dev))
    inst.scores = torch.linspace(0.95, 0.6, len(boxes), device=dev)
    inst.pred_classes = torch.zeros((len(boxes),), dtype=torch.int64, device=dev)
    inst.tag = torch.arange(len(boxes), device=dev)
    out = runner.post_processor(inst)
    assert len(out) == len(boxes)
    _assert_fields(out, "__call__")
    src = out.tag.tolist()                                             # which input word each output row is
    assert [ref["line_id"][k] for k in src] == out.pred_line_ids.tolist()
    out.pred_texts = [f"w{k}" for k in src]
    assert [ln["text"] for ln in lines_of(out)] == [" ".join(f"w{k}" for k in ref["order"][a:b])
                                                    for a, b in zip(ref["line_start"][:-1], ref["line_start"][1:])]
    first = out[out.pred_line_ids == 0]                                # filtering keeps the fields in step
    assert [ln["text"] for ln in lines_of(first)] == [" ".join(f"w{k}" for k in ref["order"][:ref["line_start"][1]])]
