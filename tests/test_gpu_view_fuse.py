"""GPU: glass_fuse_views (csrc/view_fuse.hip) against the float64 reference of tests/view_fuse_cases.py - source slots, votes,
view masks, counts and flags exactly; boxes, scores and keys bit for bit.  Every direct call of the C entry point puts guard
bands around each buffer (inputs, outputs, workspace) and confirms they are intact, and that the output rows beyond the count
still hold what the caller filled them with.  Then ops.native.fuse_views' refusals, and GlassRunner.run_views against
run_batch and against the same steps done by hand."""
import os

import numpy as np
import pytest
import torch

import view_fuse_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                      # bytes on each side of every buffer
GUARD_BYTE = 0xA5
FILL_F, FILL_I = 7.25, -5        # what the output rows hold before the call
INF = float("inf")


def _dev():
    return torch.device("cuda:0")


class Guarded:
    """a device buffer with a guard band on each side; .ptr is the address between them, read() checks the bands"""

    def __init__(self, host: np.ndarray):
        host = np.ascontiguousarray(host)
        self.dtype, self.shape, self.nbytes = host.dtype, host.shape, host.nbytes
        body = (max(host.nbytes, 1) + 15) // 16 * 16
        raw = np.full((2 * GUARD + body,), GUARD_BYTE, dtype=np.uint8)
        raw[GUARD:GUARD + host.nbytes] = host.reshape(-1).view(np.uint8)
        self.raw = torch.from_numpy(raw).to(_dev())
        self.body = body

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def read(self):
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == GUARD_BYTE).all() and (raw[GUARD + self.nbytes:] == GUARD_BYTE).all(), "a guard band was written"
        return raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def _call(case, rank="detection", min_votes=1, max_out=None, affine=None, bounds=None, counts=None, rows=None):
    """the C entry point on guarded buffers -> dict of numpy outputs (all `rows` rows of each, rows >= max_out)"""
    from glass_amd import _lib
    from glass_amd.ops import native as K
    L = _lib.lib()
    V, Kk = case["V"], case["K"]
    mode = C.MODES[rank]
    max_out = case["max_out"] if max_out is None else max_out
    rows = max_out if rows is None else rows
    ins = [Guarded(case["boxes"]), Guarded(case["scores"]), Guarded(case["counts"] if counts is None else np.asarray(counts, dtype=np.int32))]
    text = [Guarded(case["text_arg"]), Guarded(case["text_max"])] if mode else [None, None]
    frames = [Guarded(np.asarray(case["affine"] if affine is None else affine, dtype=np.float64)),
              Guarded(np.asarray(case["bounds"] if bounds is None else bounds, dtype=np.float32))]
    outs = {"boxes": Guarded(np.full((rows, 5), FILL_F, dtype=np.float32)), "scores": Guarded(np.full((rows,), FILL_F, dtype=np.float32)),
            "keys": Guarded(np.full((rows,), FILL_F, dtype=np.float32)), "src": Guarded(np.full((rows,), FILL_I, dtype=np.int32)),
            "votes": Guarded(np.full((rows,), FILL_I, dtype=np.int32)), "views": Guarded(np.full((rows,), FILL_I, dtype=np.int64)),
            "count": Guarded(np.full((3,), FILL_I, dtype=np.int32))}
    nb = int(L.glass_fuse_views_workspace_bytes(V, Kk))
    assert nb > 0
    ws = Guarded(np.zeros((nb,), dtype=np.uint8))
    _lib.check(L.glass_fuse_views(*[g.ptr for g in ins], *[None if g is None else g.ptr for g in text], case.get("T", 1),
                                  case.get("stop_index", 0), mode, *[g.ptr for g in frames], V, Kk, case["nms_thresh"], min_votes,
                                  max_out, *[g.ptr for g in outs.values()], ws.ptr, nb, K.stream_handle()), "glass_fuse_views")
    torch.cuda.synchronize()
    for g in ins + [t for t in text if t is not None] + frames + [ws]:
        g.read()
    return {k: g.read() for k, g in outs.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_matches(out, ref, what):
    n = ref["count"]
    print(f"[fuse_views] {what}: {ref['candidates']} candidates -> {ref['kept']} kept, {n} rows, flag {ref['flag']}; "
          f"kernel {out['count'].tolist()}")
    assert out["count"].tolist() == [n, ref["flag"], ref["kept"]], what
    assert np.array_equal(out["src"][:n], ref["src"]), what
    assert np.array_equal(out["votes"][:n], ref["votes"]), what
    assert np.array_equal(out["views"][:n], ref["views"]), what
    assert np.array_equal(_bits(out["scores"][:n]), _bits(ref["scores"])), what
    assert np.array_equal(_bits(out["keys"][:n]), _bits(ref["keys"])), what
    assert np.array_equal(_bits(out["boxes"][:n]), _bits(ref["boxes"])), what
    # rows beyond the count are left as the caller filled them
    assert (out["boxes"][n:] == FILL_F).all() and (out["scores"][n:] == FILL_F).all() and (out["keys"][n:] == FILL_F).all(), what
    assert (out["src"][n:] == FILL_I).all() and (out["votes"][n:] == FILL_I).all() and (out["views"][n:] == FILL_I).all(), what


def _check(case, what, **kw):
    ref_kw = {k: v for k, v in kw.items() if k in ("rank", "min_votes", "max_out")}
    ref = C.ref_of(case, **ref_kw) if ref_kw else case["ref"]
    out = _call(case, **kw)
    _assert_matches(out, ref, what)
    return out, ref


# ------------------------------------------------------------------------------------------------ the kernel
def test_one_identity_view():
    case = C.one_view_identity()
    out, _ = _check(case, "one identity view")
    assert out["count"].tolist() == [37, 0, 37] and out["src"][:37].tolist() == list(range(37))
    assert np.array_equal(_bits(out["boxes"][:37]), _bits(case["boxes"][0, :37]))
    assert np.array_equal(_bits(out["scores"][:37]), _bits(case["scores"][0, :37]))
    assert (out["votes"][:37] == 1).all() and (out["views"][:37] == 1).all()


@pytest.mark.parametrize("rank", ["detection", "product", "word"])
def test_scene_seen_by_four_rotations(rank):
    case = C.scene_four_rotations()
    for min_votes in (1, 2, 3, 4):
        out, ref = _check(case, f"40 words, four rotations, rank {rank}, min_votes {min_votes}", rank=rank, min_votes=min_votes)
        assert out["count"][2] == len(case["held"]) and (out["votes"][:ref["count"]] >= min_votes).all()


@pytest.mark.parametrize("T", [1, 26, 64])
def test_word_score_equals_the_post_processors(T):
    """rank "word": the keys are, bit for bit, the text_score that postprocess_words gives the same rows - stop symbol at step
    0, mid-word and never"""
    from glass_amd.ops import native as K
    dev = _dev()
    g = np.random.default_rng(100 + T)
    R, Cc, stop = 48, 40, 1
    prob = g.uniform(0.0, 0.2, (1, R, T, Cc)).astype(np.float32)
    for r in range(R):
        n = (0, T // 2, T)[r % 3] if T > 1 else (0, T)[r % 2]            # the step of the stop symbol; T: none
        for t in range(T):
            prob[0, r, t, stop if t == n else int(g.integers(2, Cc))] = np.float32(g.uniform(0.75, 1.0))
    boxes = np.array([[[60.0 + 70 * (r % 8), 40.0 + 40 * (r // 8), 40.0, 14.0, 0.0] for r in range(R)]], dtype=np.float32)
    scores = g.permutation(np.linspace(0.5, 0.95, R)).astype(np.float32)[None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    counts = torch.tensor([R], dtype=torch.int32, device=dev)
    arg, mx = K.text_argmax(t(prob), counts)
    words = K.postprocess_words(t(boxes), t(scores), counts, t(prob), None, [2.0, 0.15, 0.25, 0.3, 0.35, 15.0, 0.01, 0.0], stop)
    assert int(words["count"][0]) == R
    ts = np.zeros((R,), dtype=np.float32)
    ts[words["src"][0].cpu().numpy()] = words["text_score"][0].cpu().numpy()
    case = dict(boxes=boxes, scores=scores, counts=np.array([R], dtype=np.int32), affine=np.array([C.IDENTITY]), bounds=np.array(C.FREE, dtype=np.float32),
                nms_thresh=0.5, max_out=64, V=1, K=R, T=T, stop_index=stop, text_arg=arg.cpu().numpy(), text_max=mx.cpu().numpy())
    assert len(set(ts.tolist())) == R                                   # distinct keys: the order is decided
    for rank in ("word", "product"):
        out, ref = _check(case, f"T = {T}, rank {rank}", rank=rank)
        assert ref["count"] == R
        got = np.zeros((R,), dtype=np.float32)
        got[out["src"][:R]] = out["keys"][:R]
        with np.errstate(all="ignore"):
            want = ts if rank == "word" else (scores[0] * ts).astype(np.float32)
        assert np.array_equal(_bits(got), _bits(want)), rank


def test_same_view_pairs_and_the_earliest_kept():
    case = C.same_view_pairs()
    out, ref = _check(case, "IoU 0.9 pairs inside one view, a third view over both")
    assert out["count"][0] == 2 * case["pairs"] + 10


def test_ties_are_ordered_by_view_then_slot():
    _check(C.ties(), "ties")


@pytest.mark.parametrize("cands,survivors", C.CHUNK_TOTALS)
def test_chunk_boundaries(cands, survivors):
    case = C.chunks(cands, survivors)
    out, _ = _check(case, f"{cands} candidates, {survivors} survivors")
    assert out["count"].tolist() == [survivors, 0, survivors]
    _check(case, f"{cands} candidates, min_votes 2", min_votes=2)
    _check(case, f"{cands} candidates, max_out {survivors - 1}", max_out=survivors - 1)


def test_supporters_in_later_chunks():
    case = C.late_supporters()
    for mv in (1, 2, 3):
        _check(case, f"100 words, supporters one and two chunks later, min_votes {mv}", min_votes=mv)


def test_view_63_sets_the_sign_bit():
    case = C.view_63()
    out, ref = _check(case, "V = 64, K = 128")
    n = ref["count"]
    assert (out["views"][:n] < 0).all() and (out["views"][:n].view(np.uint64) >> np.uint64(63) == 1).all()
    _check(case, "V = 64, K = 128, min_votes 4", min_votes=4)


def test_exactly_1024_kept_and_one_more():
    exact = C.keep_exact()
    out, _ = _check(exact, "1124 candidates, exactly 1024 kept, nothing after")
    assert out["count"].tolist() == [1024, 0, 1024]
    cut = C.keep_cut()
    out, _ = _check(cut, "1125 candidates, the walk cut at the 1024th kept")
    assert out["count"].tolist() == [1024, 1, 1024]
    out, ref = _check(cut, "the same, min_votes 2", min_votes=2)
    assert out["count"].tolist() == [ref["count"], 1, 1024] and 0 < ref["count"] <= 100


def test_more_rows_than_max_out_after_the_vote_filter():
    case = C.late_supporters()
    out, ref = _check(case, "min_votes 2, max_out 10", min_votes=2, max_out=10)
    assert out["count"].tolist() == [10, 1, 100] and ref["cut"] == 0
    out, _ = _check(case, "max_out 1", max_out=1)
    assert out["count"].tolist() == [1, 1, 100]
    full = C.ref_of(case, min_votes=3)
    out, _ = _check(case, "min_votes 3, max_out = n", min_votes=3, max_out=full["count"])
    assert out["count"].tolist() == [full["count"], 0, 100]
    one = C.one_view_identity()
    out, _ = _check(dict(one, counts=np.array([1], dtype=np.int32)), "one candidate, max_out 1", max_out=1)
    assert out["count"].tolist() == [1, 0, 1]


def test_counts_edges():
    case = C.counts_edges()
    _check(case, "counts 0, negative, above K")
    empty = dict(case, counts=np.zeros((4,), dtype=np.int32))
    out = _call(empty)
    assert out["count"].tolist() == [0, 0, 0] and (out["src"] == FILL_I).all()


def test_nonfinite_rows_are_no_candidates():
    case = C.nonfinite_rows()
    for rank in ("detection", "product", "word"):
        _check(case, f"NaN / inf / empty rows, rank {rank}", rank=rank)


@pytest.mark.parametrize("entry", [0, 2, 4, 6, 7])
@pytest.mark.parametrize("bad", [float("nan"), INF])
def test_a_nonfinite_affine_row_drops_only_its_view(entry, bad):
    case = C.bad_affine_row()
    aff = case["affine"].copy()
    aff[1, entry] = bad
    poisoned = dict(case, affine=aff)
    ref = C.ref_of(poisoned)
    assert ref["candidates"] == 24 and ref["count"] == 12 and set((ref["src"] // case["K"]).tolist()) <= {0, 2}
    assert ref["views"].tolist() == [0b101] * 12
    _assert_matches(_call(poisoned), ref, f"view 1's entry {entry} = {bad}")


def test_bounds():
    case = C.on_the_bounds()
    out, ref = _check(case, "centres on the bounds and one ulp outside")
    assert sorted(out["src"][:ref["count"]].tolist()) == [i for i, ok in enumerate(case["inside"]) if ok]
    scene = C.scene_four_rotations()
    n_all = int(scene["counts"].sum())
    for b in ((-INF, -INF, INF, INF), (-INF, 0.0, INF, 300.0), (0.0, -INF, 420.0, INF), (100.0, -INF, INF, 200.0)):
        sub = dict(scene, bounds=np.array(b, dtype=np.float32))
        assert C.margin_violations(sub) == []
        out, ref = _check(sub, f"bounds {b}", max_out=1024)
        if b[0] == -INF and b[1] == -INF:
            assert ref["candidates"] == n_all                          # the fill-corner detections come through
    out = _call(dict(scene, bounds=np.array((np.nan, 0.0, 420.0, 300.0), dtype=np.float32)))
    assert out["count"].tolist() == [0, 0, 0]


def test_no_views():
    from glass_amd.ops import native as K
    case = dict(boxes=np.zeros((0, 8, 5), dtype=np.float32), scores=np.zeros((0, 8), dtype=np.float32), counts=np.zeros((0,), dtype=np.int32),
                affine=np.zeros((0, 8)), bounds=np.array(C.FREE, dtype=np.float32), nms_thresh=0.5, max_out=16, V=0, K=8)
    out = _call(case)
    assert out["count"].tolist() == [0, 0, 0] and (out["boxes"] == FILL_F).all() and (out["views"] == FILL_I).all()
    dev = _dev()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    out = K.fuse_views(z(0, 8, 5), z(0, 8), torch.zeros((0,), dtype=torch.int32, device=dev),
                       torch.zeros((0, 8), dtype=torch.float64, device=dev), z(4), 0.5, max_out=16)
    assert out["count"].tolist() == [0, 0, 0] and not out["boxes"].any() and tuple(out["boxes"].shape) == (16, 5)


def test_rows_beyond_max_out_and_two_runs():
    """buffers larger than max_out keep their tail, and two runs give the same bytes"""
    case = C.scene_four_rotations()
    a = _call(case, rank="product", max_out=24, rows=40)
    b = _call(case, rank="product", max_out=24, rows=40)
    ref = C.ref_of(case, "product", 1, 24)
    assert ref["count"] == 24 and ref["flag"] == 1
    _assert_matches(a, ref, "max_out 24 of 40 rows")
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    big = C.keep_cut()
    a, b = _call(big), _call(big)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _wrapper_args(case, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return dict(dict(boxes=t(case["boxes"]), scores=t(case["scores"]), counts=t(case["counts"]), view_affine=t(case["affine"]),
                     bounds=t(case["bounds"]), nms_thresh=case["nms_thresh"], text_arg=t(case["text_arg"]), text_max=t(case["text_max"]),
                     stop_index=case["stop_index"]), **kw)


def test_wrapper_matches_and_refuses():
    from glass_amd.ops import native as K
    case = C.scene_four_rotations()
    for rank in ("detection", "product", "word"):
        out = K.fuse_views(**_wrapper_args(case, rank=rank, min_votes=2, max_out=64))
        assert tuple(out) == ("boxes", "scores", "keys", "src", "votes", "views", "count")
        assert out["views"].dtype == torch.int64 and out["count"].dtype == torch.int32 and tuple(out["count"].shape) == (3,)
        ref = C.ref_of(case, rank, 2, 64)
        n = ref["count"]
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert got["count"].tolist() == [n, ref["flag"], ref["kept"]]
        for k in ("src", "votes", "views"):
            assert np.array_equal(got[k][:n], ref[k]), (rank, k)
        for k in ("boxes", "scores", "keys"):
            assert np.array_equal(_bits(got[k][:n]), _bits(ref[k])), (rank, k)
        for k in ("boxes", "scores", "keys", "src", "votes", "views"):
            assert not got[k][n:].any(), (rank, k)                      # the zeroed buffer
    good = _wrapper_args(case, rank="product")
    no_text = {k: v for k, v in _wrapper_args(case).items() if not k.startswith("text_")}
    K.fuse_views(**no_text)                                              # rank "detection" needs no text rows
    bad = [("boxes", good["boxes"].double()), ("boxes", good["boxes"].cpu()), ("boxes", good["boxes"][:, :, :4].contiguous()),
           ("boxes", good["boxes"].reshape(-1, 5)), ("boxes", good["boxes"].transpose(0, 1)), ("boxes", None),
           ("scores", good["scores"][:, :7].contiguous()), ("scores", good["scores"].half()),
           ("counts", good["counts"].long()), ("counts", good["counts"][:3].contiguous()), ("counts", good["counts"].cpu()),
           ("view_affine", good["view_affine"].float()), ("view_affine", good["view_affine"][:, :6].contiguous()),
           ("view_affine", good["view_affine"].cpu()), ("bounds", good["bounds"].double()), ("bounds", good["bounds"][:3].contiguous()),
           ("bounds", good["bounds"].cpu()), ("text_arg", None), ("text_max", None), ("text_arg", good["text_arg"].long()),
           ("text_max", good["text_max"].double()), ("text_arg", good["text_arg"][:, :, :3].contiguous()),
           ("text_max", good["text_max"][:, :5].contiguous()), ("text_arg", good["text_arg"].cpu()),
           ("rank", "best"), ("rank", 1), ("max_out", 0), ("max_out", 1025), ("min_votes", 0), ("min_votes", 65),
           ("stop_index", -1), ("nms_thresh", float("nan")), ("nms_thresh", INF)]
    for name, val in bad:
        with pytest.raises(ValueError, match="fuse_views"):
            K.fuse_views(**dict(good, **{name: val}))
    with pytest.raises(ValueError, match="fuse_views"):                  # text rows given to rank "detection" are checked too
        K.fuse_views(**dict(good, rank="detection", text_max=None))
    dev = _dev()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    for V, Kk in ((9, 1024), (65, 8), (82, 100), (2, 1025)):
        with pytest.raises(ValueError, match="V \\* K <= 8192"):
            K.fuse_views(z(V, Kk, 5), z(V, Kk), torch.zeros((V,), dtype=torch.int32, device=dev),
                         torch.zeros((V, 8), dtype=torch.float64, device=dev), z(4), 0.5)
    big = torch.zeros((2, 8, 65), device=dev)
    with pytest.raises(ValueError, match="T=65"):
        K.fuse_views(z(2, 8, 5), z(2, 8), torch.zeros((2,), dtype=torch.int32, device=dev), torch.zeros((2, 8), dtype=torch.float64, device=dev),
                     z(4), 0.5, big.int(), big, rank="word")


# ------------------------------------------------------------------------------------------------ the runner
def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"] + list(opts))


RUNNER_OPTS = ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 240, "POST_PROCESSING.TEXT_THRESHOLD", 0.0]
FIELDS = ("scores", "pred_classes", "pred_text_prob", "orientations", "pred_text_dist", "pred_polygons", "pred_text_scores",
          "pred_mask_rois", "pred_mask_boxes",
          "pred_view_votes", "pred_view", "pred_view_mask", "pred_line_ids", "pred_reading_rank", "pred_line_boxes")


@pytest.fixture(scope="module")
def runner():
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    return GlassRunner(None, None, cfg=_cfg(RUNNER_OPTS), state_dict=make_state_dict(1234), post_process=True)


def _same_instances(a, b, what, skip=()):
    assert len(a) == len(b), (what, len(a), len(b))
    assert a.image_size == b.image_size, what
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor), what
    for name in FIELDS:
        if name in skip:
            continue
        assert a.has(name) == b.has(name), (what, name)
        if a.has(name):
            assert torch.equal(a.get(name), b.get(name)), (what, name)
    if a.has("pred_texts") or b.has("pred_texts"):
        assert a.pred_texts == b.pred_texts, what


VIEW_FIELDS = ("pred_view_votes", "pred_view", "pred_view_mask")


def test_run_views_with_one_upright_view_equals_run_batch(runner):
    """images the resize policy leaves alone, and whose detections (synthetic weights: arbitrary boxes) all have their centre
    inside the image - run_views drops a centre outside its bounds, run_batch does not, and that is not what is compared here"""
    from glass_amd.utils.synth import make_image
    for seed, (h, w) in ((1, (200, 168)), (1, (176, 240)), (5, (240, 200))):
        img = make_image(seed, h, w).numpy()
        assert runner.get_inference_scale_ratio(img.shape) == 1
        det = runner.model([{"image": runner._image_at_scale(img, 1), "height": h, "width": w}]).batch
        b = det.boxes[0, :int(det.counts_host[0])]
        assert len(b) > 0 and bool(((b[:, 0] >= 0) & (b[:, 0] <= w) & (b[:, 1] >= 0) & (b[:, 1] <= h)).all()), (seed, h, w)
        ref = runner.run_batch([img])[0]
        got = runner.run_views(img, angles=(0,), scales=(1,), rank="detection")
        assert len(ref) > 0
        print(f"[run_views = run_batch] {h} x {w}: {len(ref)} words")
        _same_instances(got, ref, (h, w), skip=VIEW_FIELDS)
        assert set(got.get_fields()) - set(ref.get_fields()) == set(VIEW_FIELDS)
        assert (got.pred_view_votes == 1).all() and (got.pred_view == 0).all() and (got.pred_view_mask == 1).all()


def _by_hand(runner, img, angles, scales, rank, min_votes, post_process, batch_size, nms_thresh=None, with_masks=False):
    """run_views' steps, spelled out: rotate and resize per view, the model on groups of one padded shape, the rows put back in
    view order, K.text_argmax, K.fuse_views, the gathers, process_padded"""
    from glass_amd.inference.view_fusion import plan_views
    from glass_amd.ops import native as K
    from glass_amd.structures.core import Instances, RotatedBoxes
    dev = runner.device
    H, W = img.shape[:2]
    views = plan_views(H, W, angles, scales, runner.get_inference_scale_ratio)
    V = len(views)
    u8 = torch.from_numpy(np.ascontiguousarray(runner._grey(img))).to(dev)
    inputs = []
    for v in views:
        rot = u8 if v.rotation.angle == 0.0 else K.rotate_u8(u8, v.rotation, (0, 0, 0))
        t = runner._image_at_scale(rot, v.rho)
        inputs.append({"image": t, "height": t.shape[1], "width": t.shape[2]})
    d = runner.model.backbone.size_divisibility
    shapes = [(-(-i["height"] // d) * d, -(-i["width"] // d) * d) for i in inputs]
    Kd = int(runner.cfg.TEST.DETECTIONS_PER_IMAGE)
    T, Cc = runner.cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH + 1, len(runner.cfg.MODEL.ROI_RECOGNIZER_HEAD.CHARACTER_SET) + 2
    row = {name: [None] * V for name in ("boxes", "scores", "orient", "text", "counts_dev") + (("mask_rois",) if with_masks else ())}
    tails = {"boxes": (5,), "scores": (), "orient": (2,), "text": (T, Cc), "mask_rois": (28, 28)}
    for shape in dict.fromkeys(shapes):
        idxs = [i for i in range(V) if shapes[i] == shape]
        for c0 in range(0, len(idxs), batch_size):
            call = idxs[c0:c0 + batch_size]
            det = runner.model([inputs[i] for i in call]).batch
            for j, i in enumerate(call):
                for name in row:
                    t = getattr(det, name)
                    row[name][i] = t[j] if t is not None else torch.zeros((Kd,) + tails[name], device=dev)
    boxes, scores, orient, text, counts = (torch.stack(row[n], 0).contiguous() for n in ("boxes", "scores", "orient", "text", "counts_dev"))
    arg, mx = K.text_argmax(text, counts)
    f = lambda a, dt: torch.tensor(a, dtype=dt).to(dev)
    m = K.fuse_views(boxes, scores, counts, f([list(v.affine) for v in views], torch.float64), f([0.0, 0.0, float(W), float(H)], torch.float32),
                     float(runner.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST if nms_thresh is None else nms_thresh), arg, mx, runner.post_processor.text_encoder.character.index("[s]"),
                     rank, min_votes, 1024)
    src = m["src"].long()
    orient, text = orient.reshape(V * Kd, 2)[src][None], text.reshape(V * Kd, T, Cc)[src][None]
    n = int(m["count"][0])
    view_rows = {"pred_view_votes": m["votes"].long()[None], "pred_view": (src // Kd)[None], "pred_view_mask": m["views"][None]}
    if with_masks:           # the RoI mask rows of the kept copies, and the fused boxes as their frame
        rois = torch.stack(row["mask_rois"], 0).reshape(V * Kd, 28, 28)[src][None]
        view_rows.update({"pred_mask_rois": rois, "pred_mask_boxes": m["boxes"][None]})
    if post_process:
        one = torch.ones((1, 2), dtype=torch.float32, device=dev)
        extra = dict({"orientations": orient, "pred_text_dist": None}, **view_rows)
        return runner.post_processor.process_padded(m["boxes"][None], m["scores"][None], m["count"][:1], text, one, [(H, W)], extra)[0], n, m
    r = Instances((H, W))
    r.pred_boxes, r.scores = RotatedBoxes(m["boxes"][:n]), m["scores"][:n]
    r.pred_classes = torch.zeros((n,), dtype=torch.int64, device=dev)
    r.orientations, r.pred_text_prob = orient[0, :n], text[0, :n]
    for k, t in view_rows.items():
        r.set(k, t[0, :n])
    return r, n, m


def _popcount(t):
    return torch.tensor([bin(int(v) & (2 ** 64 - 1)).count("1") for v in t.tolist()], dtype=torch.int64)


@pytest.mark.parametrize("batch_size", [8, 1])
def test_run_views_equals_the_steps_by_hand(runner, batch_size):
    from glass_amd.utils.synth import make_image
    img = make_image(3, 160, 224).numpy()
    angles, scales = (0.0, 90.0, 180.0, 270.0), (1.0, 0.75)
    counts_seen = []
    for rank, min_votes, thr in (("product", 1, None), ("word", 2, 0.2), ("detection", 1, 0.0)):     # 0.0: given, not the config's
        ref, n, m = _by_hand(runner, img, angles, scales, rank, min_votes, True, batch_size, thr)
        got = runner.run_views(img, angles=angles, scales=scales, rank=rank, min_votes=min_votes, nms_thresh=thr, batch_size=batch_size)
        kept = int(m["count"][2])
        print(f"[run_views = by hand] rank {rank}, min_votes {min_votes}, batch_size {batch_size}: 8 views, {kept} distinct, {n} rows, "
              f"{len(ref)} words")
        assert n > 0 and len(ref) > 0 and kept >= n
        counts_seen.append((kept, n))
        _same_instances(got, ref, (rank, min_votes))
        assert got.image_size == (160, 224)
        votes = got.pred_view_votes.cpu()
        assert ((votes >= min_votes) & (votes <= 8)).all() and torch.equal(votes, _popcount(got.pred_view_mask.cpu()))
        assert ((got.pred_view_mask.cpu() >> got.pred_view.cpu()) & 1).all()          # the kept copy's own view is in its mask
    _, n_default, m_default = _by_hand(runner, img, angles, scales, "detection", 1, True, batch_size)
    assert counts_seen[2] != (int(m_default["count"][2]), n_default)    # the threshold that was passed decided, not the default
    raw, n2, _ = _by_hand(runner, img, angles, scales, "product", 1, False, batch_size)
    runner.post_process_flag = False
    try:
        got = runner.run_views(img, angles=angles, scales=scales, batch_size=batch_size)
    finally:
        runner.post_process_flag = True
    assert n2 == len(got) > 0
    _same_instances(got, raw, "post_process=False")
    assert torch.equal(got.pred_view_votes.cpu(), _popcount(got.pred_view_mask.cpu()))


def test_run_views_with_grouped_lines():
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_image, make_state_dict
    r = GlassRunner(None, None, cfg=_cfg(RUNNER_OPTS + ["POST_PROCESSING.GROUP_LINES", True]), state_dict=make_state_dict(1234))
    img = make_image(3, 160, 224).numpy()
    got = r.run_views(img, angles=(0.0, 180.0), min_votes=1)
    assert len(got) > 0
    for name in ("pred_line_ids", "pred_line_pos", "pred_reading_rank", "pred_line_boxes") + VIEW_FIELDS:
        assert got.has(name) and len(got.get(name)) == len(got), name
    ref, _, _ = _by_hand(r, img, (0.0, 180.0), (1.0,), "product", 1, True, 8)
    _same_instances(got, ref, "GROUP_LINES")


def test_run_views_carries_the_roi_masks_with_the_fused_boxes():
    """MASK_INFERENCE with PASTE_MASKS False: pred_mask_rois are the mask rows of the kept copies, gathered by source slot, and
    pred_mask_boxes the fused boxes - with and without the word post-processor"""
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_image, make_state_dict
    opts = RUNNER_OPTS + ["MODEL.ROI_MASK_HEAD.MASK_INFERENCE", True, "MODEL.MASK_ON", True, "MODEL.ROI_MASK_HEAD.PASTE_MASKS", False]
    r = GlassRunner(None, None, cfg=_cfg(opts), state_dict=make_state_dict(1234, parts=("backbone", "rpn", "box", "recog", "mask")))
    assert r.model.paste_masks is False
    img = make_image(3, 160, 224).numpy()
    angles = (0.0, 90.0, 180.0)
    ref, n, m = _by_hand(r, img, angles, (1.0,), "product", 1, True, 8, with_masks=True)
    got = r.run_views(img, angles=angles)
    assert n > 0 and len(got) > 0 and not got.has("pred_masks")
    _same_instances(got, ref, "PASTE_MASKS False")
    assert tuple(got.pred_mask_rois.shape) == (len(got), 28, 28) and tuple(got.pred_mask_boxes.shape) == (len(got), 5)
    fused = {b.numpy().tobytes() for b in m["boxes"][:n].cpu()}
    assert all(b.numpy().tobytes() in fused for b in got.pred_mask_boxes.cpu())           # the fused boxes, not the words'
    assert bool(got.pred_mask_rois.abs().sum() > 0)
    raw, n2, m2 = _by_hand(r, img, angles, (1.0,), "product", 1, False, 8, with_masks=True)
    r.post_process_flag = False
    try:
        got = r.run_views(img, angles=angles)
    finally:
        r.post_process_flag = True
    assert n2 == len(got) == n
    _same_instances(got, raw, "PASTE_MASKS False, post_process=False")
    assert torch.equal(got.pred_mask_boxes, m2["boxes"][:n2]) and torch.equal(got.pred_mask_boxes, got.pred_boxes.tensor)


class _ModelCalled(Exception):
    pass


def test_run_views_refusals_come_before_any_model_call(runner, monkeypatch):
    from glass_amd.utils.synth import make_image
    img = make_image(3, 160, 224).numpy()
    model, heads = runner.model, runner.model.roi_heads

    def stub(*a, **k):
        raise _ModelCalled()
    monkeypatch.setattr(type(model), "__call__", stub)
    with pytest.raises(_ModelCalled):                                   # the stub is in place: an accepted call reaches it
        runner.run_views(img, angles=(0.0,))
    wide = runner.cfg.clone()                                           # 9 views of 1024 detections: more than 8192 slots
    wide.defrost()
    wide.TEST.DETECTIONS_PER_IMAGE = 1024
    monkeypatch.setattr(runner, "cfg", wide)
    with pytest.raises(ValueError, match="8192"):
        runner.run_views(img, angles=tuple(40.0 * a for a in range(9)))
    monkeypatch.undo()
    monkeypatch.setattr(type(model), "__call__", stub)
    with pytest.raises(ValueError, match="min_votes"):
        runner.run_views(img, angles=(0.0, 90.0), min_votes=3)
    with pytest.raises(ValueError, match="min_votes"):
        runner.run_views(img, min_votes=0)
    with pytest.raises(ValueError, match="rank"):
        runner.run_views(img, rank="best")
    with pytest.raises(ValueError, match="plan_views"):
        runner.run_views(img, angles=(0.0, 360.0))
    with pytest.raises(ValueError, match="fill"):
        runner.run_views(img, fill=(0, 0, 256))
    monkeypatch.setattr(heads, "mask_inference", True, raising=False)
    with pytest.raises(NotImplementedError, match="MASK_INFERENCE"):
        runner.run_views(img)
    monkeypatch.setattr(heads, "mask_inference", False, raising=False)
    head = heads.recognizer_head
    monkeypatch.setattr(head, "image_segments", torch.zeros((8,), dtype=torch.int32, device=runner.device))
    with pytest.raises(NotImplementedError, match="image_segments"):
        runner.run_views(img)
    monkeypatch.setattr(head, "image_segments", None)
    monkeypatch.setattr(head, "char_boxes", True, raising=False)
    with pytest.raises(NotImplementedError, match="CHAR_BOXES"):
        runner.run_views(img)
    monkeypatch.setattr(head, "char_boxes", False, raising=False)
    for key, attr in (("INFLATE_RATIO", "inflate_ratio"), ("DROP_OVERLAPPING", "drop_overlapping_boxes")):
        monkeypatch.setattr(model, attr, 0.1 if attr == "inflate_ratio" else True, raising=False)
        with pytest.raises(NotImplementedError, match=key):
            runner.run_views(img)
        monkeypatch.setattr(model, attr, None, raising=False)
