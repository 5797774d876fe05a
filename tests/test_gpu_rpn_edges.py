"""GPU: K.rpn_topk_decode at its edges, alone and chained into K.rotated_nms_select.

Reference for every case: torch's stable descending sort on the CPU for the order, oracle.d2ops.apply_deltas_rotated on
rotated_grid_anchors for the decode, oracle.d2ops.find_top_rrpn_proposals for the chained cases.  Layout as in
test_gpu_f_ops.test_rpn_topk_decode_matches_stable_sort: N = 2, A = 12, levels (40, 52), (20, 26), (10, 13).
Scores are compared through an int32 view (NaN payloads and the sign of zero count), boxes element for element: the NaN
pattern must be the reference's, everything else within rtol 1e-5 / atol 1e-4 (equal infinities agree)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, A = 2, 12
SHAPES = [(40, 52), (20, 26), (10, 13)]
WEIGHTS = (1.0, 1.0, 1.0, 1.0, 2.0)
ANGLES = (-90, -45, 0, 45)
RPN_TOPK_MAX, RPN_TIE_CAP = 2048, 4096
IMAGE_HW = (160, 208)                     # level 0 at stride 4
NMS_THRESH, POST_TOPK = 0.7, 1000         # RotatedRPN.forward_batched: cfg.MODEL.RPN.NMS_THRESH / POST_NMS_TOPK_TEST


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _cells():
    from oracle import d2ops
    return [d2ops.rotated_cell_anchors(16 << i, (0.2, 0.5, 1.0), ANGLES) for i in range(len(SHAPES))]


def _random_heads(seed, shapes=SHAPES, delta_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    heads = [torch.randn((N, H, W, 6 * A), generator=g) for H, W in shapes]
    for h in heads:
        h[..., A:] *= delta_scale
    return heads


def _reference(heads, topks, shapes=SHAPES):
    """per level (sorted logits [N,k], decoded boxes [N,k,5], sorted flat indices [N,k], k)"""
    from oracle import d2ops
    cells, out = _cells(), []
    for i, ((H, W), head) in enumerate(zip(shapes, heads)):
        k = min(topks[i], H * W * A)
        lg = head[..., :A].reshape(N, -1)
        dl = head[..., A:].reshape(N, -1, 5)
        anchors = d2ops.rotated_grid_anchors(H, W, 4 << i, cells[i])
        srt, idx = lg.sort(dim=1, descending=True, stable=True)
        boxes = torch.stack([d2ops.apply_deltas_rotated(dl[n][idx[n, :k]], anchors[idx[n, :k]], WEIGHTS) for n in range(N)])
        out.append((srt[:, :k].contiguous(), boxes, idx[:, :k], k))
    return out


def _run(heads, topks, shapes=SHAPES, separate=False):
    """K.rpn_topk_decode on the merged [N,H,W,6A] heads, or (separate) on logits [N,H,W,A] and deltas [N,H,W,5A] tensors of
    their own.  Returns (boxes [N,S,5], scores [N,S], level [N,S]) on the device."""
    from glass_amd.ops import native as K
    dev = _dev()
    cells = _cells()
    levels, keep, off = [], [], 0
    for i, ((H, W), head) in enumerate(zip(shapes, heads)):
        if separate:
            lg, dl = head[..., :A].contiguous().to(dev), head[..., A:].contiguous().to(dev)
            ldl, ldd = A, 5 * A
        else:
            h = head.contiguous().to(dev)
            lg, dl, ldl, ldd = h, h.view(-1)[A:], 6 * A, 6 * A
        keep += [lg, dl]
        levels.append({"logits": lg, "deltas": dl, "ldl": ldl, "ldd": ldd, "H": H, "W": W, "stride": 4 << i,
                       "cell_anchors": cells[i].to(dev), "topk": topks[i], "slot_off": off})
        off += min(topks[i], H * W * A)
    ob = torch.zeros((N, off, 5), device=dev)
    os_ = torch.zeros((N, off), device=dev)
    ol = torch.full((N, off), -1, dtype=torch.int32, device=dev)
    K.rpn_topk_decode(levels, N, A, 0.0, WEIGHTS, ob, os_, ol)
    torch.cuda.synchronize()
    return ob, os_, ol


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_boxes(got, want, what):
    got, want = got.numpy(), want.numpy()
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN pattern differs at {np.argwhere(nan_g != nan_w)[:8].tolist()}"
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4, err_msg=what)


def _check(out, refs, what=""):
    ob, os_, ol = [t.cpu() for t in out]
    off = 0
    for i, (srt, boxes, _, k) in enumerate(refs):
        assert torch.equal(_bits(os_[:, off:off + k]), _bits(srt)), f"{what} level {i}: selected logits / order differ"
        _assert_boxes(ob[:, off:off + k], boxes, f"{what} level {i}")
        assert (ol[:, off:off + k] == i).all()
        off += k


# ------------------------------------------------------------------------------------------------ special logits
def _special_logit_heads():
    """level 0: NaN and +inf inside the top k, the k-th place inside a run of +0.0 / -0.0 (a tie: lower index first, the sign
    of each zero kept); level 1: more NaN than k (the k-th place is a NaN; NaN sort first, lower index first);
    level 2: +inf on top, the k-th place inside a run of -inf."""
    heads = _random_heads(21)
    g = torch.Generator().manual_seed(22)
    nan, inf = float("nan"), float("inf")
    for n in range(N):
        # level 0, k = 1000: 3 NaN + 2 inf + 980 positive < 1000 <= ... + 30 zeros; everything else negative
        H, W = SHAPES[0]
        tot = H * W * A
        perm = torch.randperm(tot, generator=g)
        v = -torch.rand(tot, generator=g) - 0.5
        v[perm[:3]] = nan
        v[perm[3:5]] = inf
        v[perm[5:985]] = torch.rand(980, generator=g) + 0.5
        zeros = torch.zeros(30)
        zeros[torch.randperm(30, generator=g)[:15]] = -0.0
        v[perm[985:1015]] = zeros
        heads[0][n, ..., :A] = v.view(H, W, A)
        # level 1, k = 1000: 1200 NaN
        H, W = SHAPES[1]
        tot = H * W * A
        perm = torch.randperm(tot, generator=g)
        v = torch.randn(tot, generator=g)
        v[perm[:1200]] = nan
        heads[1][n, ..., :A] = v.view(H, W, A)
        # level 2 (1560 anchors), k = 1000: 10 inf, 1100 -inf, 450 finite
        H, W = SHAPES[2]
        tot = H * W * A
        perm = torch.randperm(tot, generator=g)
        v = torch.randn(tot, generator=g)
        v[perm[:10]] = inf
        v[perm[10:1110]] = -inf
        heads[2][n, ..., :A] = v.view(H, W, A)
    return heads


def test_special_logits_sort_like_torch():
    """NaN, +inf, -inf, +0.0 and -0.0 inside the top k and at the k-th place: scores bit-equal to torch's stable descending sort
    (NaN first, then +inf; +0.0 and -0.0 tie and keep their index order and their sign), boxes decoded for the same anchors."""
    heads = _special_logit_heads()
    topks = [1000] * 3
    refs = _reference(heads, topks)
    # the layout really puts the specials where the docstring says (a check of the test's own construction)
    s0, s1, s2 = refs[0][0], refs[1][0], refs[2][0]
    assert torch.isnan(s0[:, :3]).all() and torch.isinf(s0[:, 3:5]).all() and (s0[:, 985:] == 0).all()
    assert (_bits(s0[:, 985:]) != 0).any() and (_bits(s0[:, 985:]) == 0).any(), "both signs of zero among the selected ties"
    assert torch.isnan(s1).all() and (s2[:, :10] == float("inf")).all() and (s2[:, 460:] == -float("inf")).all()
    _check(_run(heads, topks), refs, "special logits")


# ------------------------------------------------------------------------------------------------ special deltas
def _f32(v):
    return np.float32(v)


def _angle_delta(target_pa, aa):
    """fp32 delta d (already divided by the angle weight) whose decode `d * 180 / pi + aa`, evaluated in fp32 in the order
    both implementations use, is exactly target_pa; None if no fp32 value within 64 ulp of the real solution does that"""
    pi32, c180 = _f32(math.pi), _f32(180.0)
    d0 = _f32((target_pa - aa) * math.pi / 180.0)
    lo = hi = d0
    cands = [d0]
    for _ in range(64):
        lo, hi = np.nextafter(lo, _f32(-np.inf)), np.nextafter(hi, _f32(np.inf))
        cands += [lo, hi]
    for d in cands:
        if _f32(_f32(d * c180) / pi32) + _f32(aa) == _f32(target_pa):
            return float(d)
    return None


ANGLE_TARGETS = (-180.0, 180.0, 540.0, -540.0, 900.0)      # pa + 180 is a multiple of 360
SC32 = float(np.float32(math.log(1000.0 / 16)))            # SCALE_CLAMP as both implementations hold it in fp32
SC32_UP = float(np.nextafter(np.float32(SC32), np.float32(np.inf)))


def _poison_rows():
    """list of (name, 5 deltas or a function of the anchor angle): one special value per row, the other slots small"""
    nan, inf = float("nan"), float("inf")
    rows = []
    for s in range(5):
        rows.append((f"nan{s}", {s: nan}))
    for s in range(5):
        rows.append((f"+inf{s}", {s: inf}))
        rows.append((f"-inf{s}", {s: -inf}))
    for s, nm in ((2, "dw"), (3, "dh")):
        rows.append((f"{nm}=clamp", {s: SC32}))
        rows.append((f"{nm}=clamp+1ulp", {s: SC32_UP}))
        rows.append((f"{nm}=100", {s: 100.0}))
    for t in ANGLE_TARGETS:
        rows.append((f"pa={t}", {4: ("angle", t)}))
    rows.append(("pa=1e6", {4: ("angle1e6", None)}))
    return rows


def _poisoned_heads(seed, delta_scale):
    """random heads in which, per image and level, the anchors of `_poison_rows` carry the largest logits (50 + j / 2 + level / 8,
    distinct over the whole image) and one special delta each.  Returns (heads, names of the poison rows)."""
    heads = _random_heads(seed, delta_scale=delta_scale)
    rows = _poison_rows()
    g = torch.Generator().manual_seed(seed + 1)
    for i, (H, W) in enumerate(SHAPES):
        tot = H * W * A
        assert (len(rows) - 1) * 4 + N < H * W                          # one cell per poisoned anchor
        for n in range(N):
            px = heads[i][n].view(H * W, 6 * A)             # a view: pixel rows of logits | deltas
            for j, (name, spec) in enumerate(rows):
                cell, a = j * 4 + 1 + n, (j + 5 * n) % A
                d = torch.randn(5, generator=g) * 0.05
                for s, v in spec.items():                   # v: the delta AFTER the division by its weight
                    if isinstance(v, tuple) and v[0] == "angle":
                        # the first anchor of the cell (from a on) whose angle admits an exact fp32 solution
                        sols = [(b % A, _angle_delta(v[1], float(ANGLES[b % 4]))) for b in range(a, a + A)]
                        sols = [(b, da) for b, da in sols if da is not None]
                        assert sols, f"no exact fp32 delta for {name}"
                        a, v = sols[0]
                    elif isinstance(v, tuple):
                        v = float(np.float32((1e6 - ANGLES[a % 4]) * math.pi / 180.0))
                    d[s] = v * WEIGHTS[s]                   # weights are powers of two: the division gives v back exactly
                px[cell, a] = 50.0 + 0.5 * j + 0.125 * i
                px[cell, A + 5 * a:A + 5 * a + 5] = d
    return heads, [r[0] for r in rows]


def test_special_deltas_at_selected_anchors():
    """NaN and +-inf in each of the five delta slots, dw / dh exactly at SCALE_CLAMP, one ulp above and far above, angle deltas
    that put pa + 180 exactly on a multiple of 360 (pa = +-180, +-540, 900) and at 1e6 degrees - at the anchors with the largest
    logits of every level.  torch.clamp(max=) keeps a NaN size delta NaN (the proposal filter then drops the row); every
    other element must agree with the reference decode."""
    heads, names = _poisoned_heads(31, 1.0)
    topks = [1000] * 3
    refs = _reference(heads, topks)
    P = len(names)
    for i, (srt, boxes, _, _) in enumerate(refs):      # the poisoned anchors are the first P selected, in reverse row order
        assert torch.equal(srt[:, :P], (50.0 + 0.125 * i + 0.5 * torch.arange(P - 1, -1, -1.0)).expand(N, P))
        for j, name in enumerate(names):
            row = boxes[:, P - 1 - j]
            if name.startswith("nan"):
                s = int(name[3])
                assert torch.isnan(row[:, s]).all() and torch.isfinite(row).sum() == 4 * N, name
            if name.startswith("pa=") and name != "pa=1e6":
                assert (row[:, 4] == -180.0).all(), (name, row[:, 4])
    _check(_run(heads, topks), refs, "special deltas")


# ------------------------------------------------------------------------------------------------ chained into the NMS select
def _chain_reference(heads, topk):
    from oracle import d2ops
    cells = _cells()
    props, logits = [], []
    for i, ((H, W), head) in enumerate(zip(SHAPES, heads)):
        anchors = d2ops.rotated_grid_anchors(H, W, 4 << i, cells[i])
        dl = head[..., A:].reshape(N, -1, 5)
        props.append(torch.stack([d2ops.apply_deltas_rotated(dl[n], anchors, WEIGHTS) for n in range(N)]))
        logits.append(head[..., :A].reshape(N, -1))
    return d2ops.find_top_rrpn_proposals(props, logits, [IMAGE_HW] * N, NMS_THRESH, topk, POST_TOPK)


def _chain_margin_violations(refs):
    """pairs of valid clipped candidates of one level whose float64 IoU is within IOU_MARGIN of the NMS threshold"""
    import detection_tail_cases as C
    from oracle import d2ops
    bad = []
    for n in range(N):
        for i, (srt, boxes, _, _) in enumerate(refs):
            b = boxes[n].clone()
            ok = torch.isfinite(b).all(dim=1) & torch.isfinite(srt[n])
            b = d2ops.clip_rotated_(b[ok], IMAGE_HW)
            b = b[(b[:, 2] > 0) & (b[:, 3] > 0)].double().numpy()
            bad += [(n, i) + p for p in C.iou_margin_violations(b, (NMS_THRESH,))]
    return bad


CHAIN_TOPK = 48


def test_poisoned_levels_through_nms_select_match_find_top_rrpn_proposals():
    """the poisoned level set of the special-delta test (48 candidates per level: the poisoned anchors plus random ones)
    through rotated_nms_select with RotatedRPN.forward_batched's arguments (score threshold -inf, NMS 0.7, top 1000,
    CLIP | DROP_EMPTY, the level as category): kept slots, boxes and scores equal find_top_rrpn_proposals.  Rows with a
    non-finite box are dropped, so a NaN size delta must still be NaN when it reaches the filter.  No pair of candidates has
    an IoU within 1e-3 of the threshold (asserted), and all logits are distinct."""
    from glass_amd.ops import native as K
    dev = _dev()
    heads, _ = _poisoned_heads(41, 0.2)
    topks = [CHAIN_TOPK] * 3
    refs = _reference(heads, topks)
    assert not _chain_margin_violations(refs), "test construction: a candidate pair sits on the NMS threshold"
    want = _chain_reference(heads, CHAIN_TOPK)
    ob, os_, ol = _run(heads, topks)
    _check((ob, os_, ol), refs, "chain candidates")
    hw = torch.tensor([IMAGE_HW] * N, dtype=torch.int32, device=dev)
    kb, ks, ki, kc = K.rotated_nms_select(ob, os_, ol, None, hw, float("-inf"), NMS_THRESH, POST_TOPK, K.NMS_CLIP | K.NMS_DROP_EMPTY)
    torch.cuda.synchronize()
    cand_scores = torch.cat([r[0] for r in refs], dim=1)
    assert all(len(torch.unique(cand_scores[n])) == cand_scores.shape[1] for n in range(N)), "test construction: logits must be distinct"
    for n, (wb, ws) in enumerate(want):
        cnt = int(kc[n])
        assert cnt == len(ws) and 0 < cnt < 3 * CHAIN_TOPK, (n, cnt, len(ws))
        assert torch.equal(_bits(ks[n, :cnt].cpu()), _bits(ws)), f"image {n}: kept scores differ"
        slots = torch.stack([torch.nonzero(_bits(cand_scores[n]) == b)[0, 0] for b in _bits(ws)])   # logits are distinct
        assert torch.equal(ki[n, :cnt].cpu().long(), slots), f"image {n}: kept slots differ"
        np.testing.assert_allclose(kb[n, :cnt].cpu().numpy(), wb.numpy(), rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------ separate heads
def test_separate_logit_and_delta_tensors_equal_the_merged_head():
    """logits as their own contiguous [N,H,W,A] tensor (ldl == A: the flat-index read of logit_key) and deltas as their own
    [N,H,W,5A] tensor (ldd == 5A): bit-equal to the merged-head call on the same values, and equal to the reference"""
    heads = _random_heads(51)
    heads[1][..., :A] = torch.round(heads[1][..., :A] * 2) / 2       # ties on one level
    topks = [1000] * 3
    merged = [t.cpu() for t in _run(heads, topks)]
    apart = [t.cpu() for t in _run(heads, topks, separate=True)]
    for m, s, nm in zip(merged, apart, ("boxes", "scores", "level")):
        assert torch.equal(_bits(m) if m.dtype == torch.float32 else m, _bits(s) if s.dtype == torch.float32 else s), nm
    _check(apart, _reference(heads, topks), "separate heads")


# ------------------------------------------------------------------------------------------------ exact fallback
@pytest.mark.parametrize("mode", ["low8", "equal"])
def test_fallback_below_a_non_empty_winner_list(mode):
    """more than RPN_TIE_CAP logits share the top 24 key bits of the k-th value - differing in the low 8 bits (1 + j 2^-23,
    j < 256) or bit-equal - below 300 clearly larger ones: the tie list overflows while list A is non-empty, and the exact
    64-bit select of the finalize kernel has to reproduce the stable sort"""
    heads = _random_heads(61)
    g = torch.Generator().manual_seed(62)
    H, W = SHAPES[0]
    tot = H * W * A
    n_tie = RPN_TIE_CAP + 904
    for n in range(N):
        perm = torch.randperm(tot, generator=g)
        v = torch.randn(tot, generator=g).clamp(max=0.9)
        v[perm[:300]] = 5.0 + torch.rand(300, generator=g)
        if mode == "low8":
            j = torch.randint(0, 256, (n_tie,), generator=g)
            v[perm[300:300 + n_tie]] = 1.0 + j.float() * 2.0 ** -23
        else:
            v[perm[300:300 + n_tie]] = 1.0
        heads[0][n, ..., :A] = v.view(H, W, A)
    tie_bits = _bits(heads[0][..., :A]) >> 8
    assert int((tie_bits == (0x3f800000 >> 8)).sum()) == N * n_tie
    topks = [1000] * 3
    refs = _reference(heads, topks)
    assert (refs[0][0][:, 299] >= 5.0).all() and (refs[0][0][:, 300:] < 1.0 + 2.0 ** -15).all() and (refs[0][0][:, 999] >= 1.0).all()
    _check(_run(heads, topks), refs, f"fallback {mode}")


# ------------------------------------------------------------------------------------------------ limits of k
def test_topk_equal_to_the_level_size_and_to_the_maximum():
    """topk = H*W*A (every anchor of the level comes out, NaN and -inf included, in sorted order) and topk = RPN_TOPK_MAX on
    the largest level"""
    heads = _random_heads(71)
    g = torch.Generator().manual_seed(72)
    H, W = SHAPES[2]
    tot = H * W * A
    for n in range(N):
        perm = torch.randperm(tot, generator=g)
        v = heads[2][n, ..., :A].reshape(-1).clone()
        v[perm[:4]] = float("nan")
        v[perm[4:9]] = -float("inf")
        v[perm[9:12]] = torch.tensor([0.0, -0.0, 0.0])
        heads[2][n, ..., :A] = v.view(H, W, A)
    topks = [RPN_TOPK_MAX, 1000, tot]
    refs = _reference(heads, topks)
    assert refs[0][3] == RPN_TOPK_MAX and refs[2][3] == tot == 1560
    _check(_run(heads, topks), refs, "k limits")


def test_topk_above_the_maximum_is_refused():
    """topk = 2049 on a level that has that many anchors: the library's error, nothing launched"""
    from glass_amd._lib import GlassLibraryError
    heads = _random_heads(81)
    with pytest.raises(GlassLibraryError, match="topk=2049"):
        _run(heads, [RPN_TOPK_MAX + 1, 1000, 1000])
    with pytest.raises(GlassLibraryError, match="topk=2049"):           # also when only the last level asks for it
        _run(heads, [1000, RPN_TOPK_MAX + 1, 1000])
