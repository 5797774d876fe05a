"""GPU: glass_order_lines (csrc/line_order.hip) through ops.native.order_lines against the independent checker of
line_order_cases.py - page_rank, page_order, block_id, block_start, block_count, forced and line_first exactly, block_boxes
within one float32 unit in the last place of the checker's float64 box - at every size where the kernels take another path, on
the page scenes and the hand-made ones, with padding rows of NaN and 1e30; determinism; and the post-processor with
POST_PROCESSING.ORDER_LINES through run_batch, run_tiled and __call__."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import line_order_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = C.INT_FIELDS + ("block_boxes", "block_count", "forced")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _batch(images, K):
    """line boxes float32 [N, K, 5] with the images' lines first and NaN / 1e30 rows beyond, counts int32 [N]"""
    boxes = np.empty((len(images), K, 5), dtype=np.float32)
    boxes[:, 0::2], boxes[:, 1::2] = np.nan, 1e30
    for n, b in enumerate(images):
        boxes[n, :len(b)] = b
    return boxes, np.array([len(b) for b in images], dtype=np.int32)


def _run(boxes, counts, line_start=None, **params):
    from glass_amd.ops import native as K
    dev = _dev()
    start = None if line_start is None else torch.from_numpy(np.ascontiguousarray(line_start, dtype=np.int32)).to(dev)
    out = K.order_lines(torch.from_numpy(boxes).to(dev), torch.from_numpy(counts).to(dev), start, **params)
    assert sorted(out) == sorted(KEYS + (("line_first",) if line_start is not None else ()))
    N, Kk = boxes.shape[:2]
    shapes = {"page_rank": (N, Kk), "page_order": (N, Kk), "block_id": (N, Kk), "block_start": (N, Kk + 1), "block_boxes": (N, Kk, 5),
              "block_count": (N,), "forced": (N,), "line_first": (N, Kk)}
    for k, v in out.items():
        assert tuple(v.shape) == shapes[k] and v.dtype == (torch.float32 if k == "block_boxes" else torch.int32), k
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(out, n, ref, K, what):
    want = C.expected_padded(ref, K)
    assert int(out["block_count"][n]) == want["block_count"], what
    assert int(out["forced"][n]) == want["forced"], what
    for k in C.INT_FIELDS:
        got = out[k][n].tolist()
        assert got == want[k], f"{what}, {k}: first difference at {next(i for i, (a, b) in enumerate(zip(got, want[k])) if a != b)}"
    B = ref["block_count"]
    worst = max([C.box_ulps(out["block_boxes"][n, b], ref["block_boxes"][b]) for b in range(B)], default=0)
    assert worst <= 1, f"{what}: a block box {worst} float32 ulps from the checker's"
    assert not out["block_boxes"][n, B:].view(np.uint32).any(), what          # zeros beyond the block count
    return worst


@pytest.mark.parametrize("K", C.K_LIST)
def test_sizes_with_counts_0_K_and_half(K):
    full, half = C.case(f"page of {K}" if K else "no lines"), C.case(f"page of {K // 2}" if K // 2 else "no lines")
    boxes, counts = _batch([np.zeros((0, 5), dtype=np.float32), full[1], half[1]], K)
    assert counts.tolist() == [0, K, K // 2]
    out = _run(boxes, counts)
    _check(out, 0, C.case("no lines")[3], K, f"K={K}, no lines")
    _check(out, 1, full[3], K, f"K={K}, {K} lines")
    _check(out, 2, half[3], K, f"K={K}, {K // 2} lines")
    assert out["page_order"][1, :K].tolist() == full[2]                # the order of construction


def test_the_large_scenes():
    names = ("one column of 1024", "one row of 1024", "page of 1024")
    cases = [C.case(n) for n in names]
    out = _run(*_batch([c[1] for c in cases], 1024))
    for n, (name, _, built, ref) in enumerate(cases):
        print(f"[line_order] {name}: {ref['block_count']} blocks, worst box {_check(out, n, ref, 1024, name)} ulp")
        assert out["page_order"][n].tolist() == built, name
    assert out["block_count"].tolist()[:2] == [3, 1024] and out["forced"].tolist() == [0, 0, 0]


def test_the_column_pages():
    names = ("2 columns", "3 columns", "4 columns", "2 columns at 30 degrees", "3 columns at 30 degrees", "4 columns at 30 degrees",
             "2 columns at -170 degrees", "3 columns at -170 degrees", "4 columns at -170 degrees",
             "a full-width line between two bands", "two bands of 3 columns at -170 degrees")
    cases = [C.case(n) for n in names]
    out = _run(*_batch([c[1] for c in cases], 210))
    for n, (name, boxes, built, ref) in enumerate(cases):
        _check(out, n, ref, 210, name)
        assert out["page_order"][n, :len(boxes)].tolist() == built and int(out["forced"][n]) == 0, name


def test_the_hand_made_scenes():
    names = ("identical boxes", "random overlapping boxes", "random overlapping boxes, 65", "four-line cycle", "lines that are no lines")
    cases = [C.case(n) for n in names]
    out = _run(*_batch([c[1] for c in cases], 200))
    for n, (name, _, _, ref) in enumerate(cases):
        _check(out, n, ref, 200, name)
    assert out["forced"][0] == 0 and out["forced"][1] > 0 and out["forced"][2] > 0 and out["forced"][3] == 1
    assert out["page_order"][3, :4].tolist() == [2, 3, 0, 1]
    boxes, ref = cases[4][1], cases[4][3]
    for k in range(len(boxes)):                                        # an invalid line's block box: its own bits
        if not ref["valid"][k]:
            assert out["block_boxes"][4, out["block_id"][4, k]].view(np.uint32).tolist() == boxes[k].view(np.uint32).tolist()


def test_counts_are_clamped_and_thresholds_reach_the_kernel():
    name, b, built, ref = C.case("page of 64")
    boxes, counts = _batch([b, b, b], 64)
    out = _run(boxes, np.array([64 + 7, -3, 64], dtype=np.int32))
    _check(out, 0, ref, 64, "count above K")
    _check(out, 1, C.case("no lines")[3], 64, "negative count")
    _check(out, 2, ref, 64, "count = K")
    two = np.array([[100, 100, 200, 20, 0], [100, 130, 200, 12, 0]], dtype=np.float32)
    side = np.array([[300, 100, 200, 20, 0], [120, 108, 200, 20, 0]], dtype=np.float32)
    for scene, params, blocks, order in ((two, {}, 2, [0, 1]), (two, {"block_min_height_ratio": 0.5}, 1, [0, 1]),
                                         (two, {"block_min_height_ratio": 0.5, "block_max_gap": 0.4}, 2, [0, 1]),
                                         (side, {"min_overlap": 0.2}, 2, [1, 0]), (side, {"min_overlap": 0.05}, 1, [0, 1])):
        out = _run(*_batch([scene], 2), **params)
        _check(out, 0, C.reference(scene, dict(C.DEFAULTS, **params)), 2, str(params))
        assert int(out["block_count"][0]) == blocks and out["page_order"][0].tolist() == order, params


def test_errors_before_any_launch_and_empty_batches():
    from glass_amd.ops import native as K
    dev = _dev()
    b, c = torch.zeros((1, 4, 5), device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        for bad in ({"min_overlap": float("nan")}, {"min_overlap": 1.0}, {"block_max_gap": -1}, {"block_min_height_ratio": 1.5}):
            with pytest.raises(ValueError):
                K.order_lines(b, c, **bad)
        with pytest.raises(ValueError, match="K <= 1024"):
            K.order_lines(torch.zeros((1, 1025, 5), device=dev), c)
        with pytest.raises(ValueError, match="line_count"):
            K.order_lines(b, torch.zeros((2,), dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match="line_count"):
            K.order_lines(b, c.cpu())
        with pytest.raises(ValueError, match="line_start"):
            K.order_lines(b, c, torch.zeros((1, 4), dtype=torch.int32, device=dev))
        with pytest.raises(K.GlassLibraryError):
            K.order_lines(b, c.long())
        with pytest.raises(K.GlassLibraryError):
            K.order_lines(b.double(), c)
        out = K.order_lines(torch.zeros((0, 8, 5), device=dev), torch.zeros((0,), dtype=torch.int32, device=dev),
                            torch.zeros((0, 9), dtype=torch.int32, device=dev))
        assert tuple(out["block_start"].shape) == (0, 9) and tuple(out["line_first"].shape) == (0, 8)       # N = 0: no launch
    out = _run(np.zeros((2, 0, 5), dtype=np.float32), np.array([0, 3], dtype=np.int32), np.zeros((2, 1), dtype=np.int32))     # K = 0
    assert out["block_start"].tolist() == [[0], [0]] and out["block_count"].tolist() == [0, 0] and out["forced"].tolist() == [0, 0]
    assert out["page_rank"].shape == (2, 0) and out["line_first"].shape == (2, 0)


def test_line_first_with_given_and_with_hostile_starts():
    cases = [C.case(n) for n in ("3 columns", "random overlapping boxes", "page of 65")]
    K = 600
    boxes, counts = _batch([c[1] for c in cases], K)
    rng = np.random.RandomState(4)
    start = np.empty((3, K + 1), dtype=np.int32)
    for n, c in enumerate(cases):
        L = len(c[1])
        s = np.concatenate([[0], np.cumsum(rng.randint(0, 4, size=L))])
        start[n, :L + 1], start[n, L + 1:] = s, s[-1]
    hostile = start.copy()
    hostile[0, 5], hostile[0, 17], hostile[0, 40] = -4, K + 9, 0
    hostile[1, 0], hostile[1, 100], hostile[1, 199] = 2 ** 31 - 1, -2 ** 31, K + 1
    hostile[2, 66:] = -99                                              # (beyond the count + 1: never read)
    for what, st in (("given", start), ("hostile", hostile)):
        out = _run(boxes, counts, st)
        for n, (name, b, _, ref) in enumerate(cases):
            _check(out, n, ref, K, f"{name}, {what} starts")
            L = len(b)
            assert out["line_first"][n, :L].tolist() == C.line_first(ref, st[n], K), (name, what)
            assert out["line_first"][n, L:].tolist() == [-1] * (K - L), (name, what)
    sizes = np.diff(start[0])[:len(cases[0][1])]
    order = out["page_order"][0, :len(sizes)]
    assert _run(boxes, counts, start)["line_first"][0, order].tolist() == np.concatenate([[0], np.cumsum(sizes[order])[:-1]]).tolist()


def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_neighbours():
    cases = [C.case(n) for n in ("page of 511", "random overlapping boxes", "3 columns at 30 degrees", "page of 129")]
    boxes, counts = _batch([c[1] for c in cases], 600)
    a, b = _run(boxes, counts), _run(boxes, counts)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for n in (0, 1):                                                   # alone, and after other neighbours
        alone = _run(boxes[n:n + 1], counts[n:n + 1])
        moved = _run(boxes[[3, 2, n]], counts[[3, 2, n]])
        for k in a:
            assert np.array_equal(alone[k][0].view(np.uint32), a[k][n].view(np.uint32)), (k, n)
            assert np.array_equal(moved[k][2].view(np.uint32), a[k][n].view(np.uint32)), (k, n)


# ------------------------------------------------------------------------------------------------ the post-processor
RUNNER_OPTS = ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "POST_PROCESSING.TEXT_THRESHOLD", 0.0,
               "POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ORDER_LINES", True]
LINE_FIELDS = ("pred_line_ids", "pred_line_pos", "pred_reading_rank", "pred_line_boxes")
NEW_FIELDS = ("pred_page_rank", "pred_block_ids", "pred_block_boxes")
COLS, ROWS, WORDS = 2, 6, 3


@pytest.fixture(scope="module")
def runner():
    from glass_amd.config import get_glass_cfg
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), RUNNER_OPTS)
    return GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)


def _two_column_page():
    """words of a two-column page, numbered in the order a reader takes them (column, row, word), then shuffled: float32
    [36, 5] and, per row of it, that number.  Rows 0-2 and 3-5 of a column are two paragraphs."""
    rows = [[80.0 + 450.0 * c + 70.0 * w, 100.0 + 34.0 * r + (60.0 if r >= 3 else 0.0) + 3.0 * c, 60.0, 20.0, 0.0]
            for c in range(COLS) for r in range(ROWS) for w in range(WORDS)]
    perm = np.random.RandomState(1).permutation(len(rows))
    return np.asarray(rows, dtype=np.float32)[perm], perm


def _assert_fields(inst, what):
    """the new fields of one Instances against the host statements and the checker on the boxes it returns"""
    from glass_amd.postprocess import blocks_of, group_lines_host, order_lines_host
    boxes = inst.pred_boxes.tensor.cpu().numpy()
    c = len(boxes)
    g = group_lines_host(boxes)
    for name in LINE_FIELDS + NEW_FIELDS:
        assert inst.has(name) and len(inst.get(name)) == c, (what, name)
    assert inst.pred_page_rank.dtype == torch.int64 and inst.pred_block_ids.dtype == torch.int64, what
    lid = inst.pred_line_ids.cpu().numpy()
    assert lid.tolist() == g["line_id"].tolist(), what
    line_boxes = np.zeros((g["line_count"], 5), dtype=np.float32)      # the line boxes the device ordered, bit for bit
    line_boxes[lid] = inst.pred_line_boxes.cpu().numpy()
    host, ref = order_lines_host(line_boxes, line_start=g["line_start"]), C.reference(line_boxes)
    assert host["page_order"].tolist() == ref["page_order"] and host["block_id"].tolist() == ref["block_id"], what
    assert inst.pred_block_ids.tolist() == [ref["block_id"][l] for l in lid], what
    first = C.line_first(ref, g["line_start"], c)
    assert inst.pred_page_rank.tolist() == [first[l] + p for l, p in zip(lid, g["line_pos"].tolist())], what
    assert sorted(inst.pred_page_rank.tolist()) == list(range(c)), what
    got = inst.pred_block_boxes.cpu().numpy()
    assert got.shape == (c, 5) and got.dtype == np.float32, what
    for k in range(c):
        assert C.box_ulps(got[k], ref["block_boxes"][ref["block_id"][lid[k]]]) <= 1, (what, k)
    blocks = blocks_of(inst)
    assert [k for b in blocks for ln in b["lines"] for k in ln["words"]] == np.argsort(inst.pred_page_rank.cpu().numpy()).tolist(), what
    assert len(blocks) == ref["block_count"], what
    return len(blocks)


def test_call_reads_a_two_column_page_column_by_column(runner):
    from glass_amd.postprocess import blocks_of, page_text
    from glass_amd.structures.core import Instances, RotatedBoxes
    boxes, number = _two_column_page()
    dev = _dev()
    inst = Instances((1200, 1200))
    inst.pred_boxes = RotatedBoxes(torch.from_numpy(boxes).to(dev))
    inst.scores = torch.linspace(0.95, 0.6, len(boxes), device=dev)
    inst.pred_classes = torch.zeros((len(boxes),), dtype=torch.int64, device=dev)
    inst.tag = torch.from_numpy(number).to(dev)
    out = runner.post_processor(inst)
    assert len(out) == len(boxes)                                      # (no word of the page is merged or dropped)
    assert _assert_fields(out, "__call__") == 2 * COLS
    built = out.tag.tolist()                                           # the reader's number of each output row
    assert out.pred_page_rank.tolist() == built                        # column by column: the order of construction
    reading = out.pred_reading_rank.tolist()                           # top to bottom: the columns interleave row by row
    per_row = COLS * WORDS
    assert reading != built
    assert [reading[built.index(k)] for k in range(WORDS * ROWS * COLS)] == \
        [per_row * r + WORDS * c + w for c in range(COLS) for r in range(ROWS) for w in range(WORDS)]
    out.pred_texts = [f"w{k}" for k in built]
    lines = [" ".join(f"w{WORDS * ROWS * c + WORDS * r + w}" for w in range(WORDS)) for c in range(COLS) for r in range(ROWS)]
    assert page_text(out) == "\n\n".join("\n".join(lines[3 * q:3 * q + 3]) for q in range(2 * COLS))
    first = out[out.pred_block_ids == 0]                               # filtering keeps the fields in step
    assert [ln["text"] for b in blocks_of(first) for ln in b["lines"]] == lines[:3]


def test_the_padded_tensors_travel_with_the_step(runner):
    page, number = _two_column_page()
    dev = _dev()
    b = np.zeros((2, 140, 5), dtype=np.float32)                        # K > 128: behind the dense word kernel
    b[0, :36], b[1, :20] = page, page[:20]
    counts = np.array([36, 20], dtype=np.int32)
    scores = torch.full((2, 140), 0.9, device=dev)
    res = runner.post_processor.process_padded(torch.from_numpy(b).to(dev), scores, torch.from_numpy(counts).to(dev), None, None,
                                               [(1200, 1200), (1200, 1200)])
    w = res.words
    assert w["count"].tolist() == [36, 20]
    for name, shape in (("page_rank", (2, 140)), ("page_order", (2, 140)), ("block_id", (2, 140)), ("block_start", (2, 141)),
                        ("block_boxes", (2, 140, 5)), ("block_count", (2,)), ("forced", (2,)), ("line_first", (2, 140)),
                        ("line_id", (2, 140)), ("order", (2, 140))):
        assert tuple(w[name].shape) == shape, name
    for n, inst in enumerate(res):
        _assert_fields(inst, f"padded {n}")
        L = int(w["line_count"][n])
        assert w["page_rank"][n, L:].tolist() == [-1] * (140 - L) and sorted(w["page_rank"][n, :L].tolist()) == list(range(L))
        assert inst.pred_block_ids.tolist() == w["block_id"][n].long()[inst.pred_line_ids].tolist()
    assert w["block_count"].tolist()[0] == 2 * COLS and w["forced"].tolist()[0] == 0
    src = w["src"][0, :36].long().cpu().numpy()
    assert res[0].pred_page_rank.tolist() == number[src].tolist()


def test_run_batch_and_run_tiled_carry_the_page_order_and_without_the_key_nothing_is_launched(runner):
    from glass_amd.ops import native as K
    from glass_amd.utils.synth import make_image
    pp = runner.post_processor
    assert pp.order_params == C.DEFAULTS and pp.line_params is not None
    imgs = [make_image(5, 100, 80).numpy(), make_image(9, 250, 180).numpy()]
    big = make_image(3, 160, 224).numpy()
    tiled = dict(tile=128, overlap=64, border=8)
    on = runner.run_batch(imgs) + [runner.run_tiled(big, **tiled)]
    words = 0
    for n, inst in enumerate(on):
        assert len(inst) > 0, n
        blocks = _assert_fields(inst, f"image {n}")
        print(f"[line_order] image {n}: {len(inst)} words in {blocks} blocks")
        words += len(inst)
    assert words >= 3
    params, pp.order_params = pp.order_params, None                    # what the constructor leaves with the key off
    try:
        with mock.patch.object(K, "order_lines", side_effect=AssertionError("launched")):
            off = runner.run_batch(imgs) + [runner.run_tiled(big, **tiled)]
    finally:
        pp.order_params = params
    for n, (a, b) in enumerate(zip(on, off)):
        fields_on, fields_off = a.get_fields(), b.get_fields()
        assert sorted(fields_on) == sorted(list(fields_off) + list(NEW_FIELDS)), n
        for name, v in fields_off.items():                             # everything else, pred_reading_rank included, bit for bit
            x = fields_on[name]
            if isinstance(v, torch.Tensor):
                assert v.dtype == x.dtype and torch.equal(v.contiguous().view(torch.uint8), x.contiguous().view(torch.uint8)), (n, name)
            elif hasattr(v, "tensor"):
                assert torch.equal(v.tensor.contiguous().view(torch.uint8), x.tensor.contiguous().view(torch.uint8)), (n, name)
            else:
                assert v == x, (n, name)
