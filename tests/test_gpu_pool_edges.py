"""GPU: rotated RoIAlign and the small streaming kernels (max pooling, image resize / preprocess, mask branch helpers) at
their edges - boundary comparisons, degenerate boxes, level boundaries, grid folds, non-finite values - against float64
restatements (tests/known_answers.py) or exact torch CPU references.  Shapes are the smallest that reach each branch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # fp32 unit roundoff


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _say(capsys, msg):
    with capsys.disabled():
        print("\n" + msg, end="")


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ================================================================================================ RoIAlign
ROI_TOL = 1e-4           # the project's RoIAlign tolerance (test_roi_align_rotated_matches_oracle)


def _roi_level(dtype):
    import pool_edge_cases as P
    feat = P.roi_features()
    lvl = torch.from_numpy(feat).to(dtype).permute(1, 2, 0).contiguous()[None].to(_dev())      # [1,H,W,C]
    assert torch.equal(lvl.cpu().double(), torch.from_numpy(feat).permute(1, 2, 0)[None])       # exact in either dtype
    return feat, lvl


def _roi_run(lvl, boxes, out_hw, sr, **kw):
    from glass_amd.ops import native as K
    dev = _dev()
    b = torch.from_numpy(np.asarray(boxes)).float().contiguous().to(dev)
    idx = torch.zeros((len(boxes),), dtype=torch.int32, device=dev)
    y = K.roi_align_rotated([lvl], [1.0], b, idx, out_hw, sr, **kw)
    torch.cuda.synchronize()
    return y


def _roi_want(feat, boxes, out_hw, sr):
    from known_answers import roi_align_rotated_f64
    return np.stack([roi_align_rotated_f64(feat, b, out_hw, 1.0, sr) for b in boxes]).transpose(0, 2, 3, 1)   # [R,PH,PW,C]


@pytest.mark.parametrize("sr,out_hw", [(1, (2, 2)), (2, (2, 2)), (1, (3, 5)), (2, (3, 5))])
def test_roi_align_sample_points_on_the_boundary(sr, out_hw, capsys):
    """axis-aligned dyadic boxes whose first / last sample row or column lies exactly on -1.5, -1 - 1/16, -1, -0.5, 0, H-1,
    H-0.5, H, H + 1/16, H + 0.5 (the same in x, and both at once): a sample is skipped when y < -1 or y > H (exclusive: -1 and
    H themselves are read, clamped), so each case pins one side of one comparison.  Against the float64 helper, 1e-4; the
    oracle's fp32 restatement is within 3.3e-7 of the helper on these inputs (tests/test_oracle_d2ops.py), far below a
    quarter of the tolerance."""
    import pool_edge_cases as P
    feat, lvl = _roi_level(torch.float32)
    cases = P.boundary_boxes(sr, out_hw)
    boxes = [b for _, b, _ in cases]
    got = _roi_run(lvl, boxes, out_hw, sr).cpu().double().numpy()
    want = _roi_want(feat, boxes, out_hw, sr)
    err = np.abs(got - want).reshape(len(boxes), -1).max(axis=1)
    _say(capsys, f"roi boundary sr={sr} out={out_hw}: max |err| {err.max():.2e}")
    assert err.max() <= ROI_TOL, [(cases[i][0], float(err[i])) for i in np.argsort(-err)[:5]]


@pytest.mark.parametrize("out_hw", [(2, 2), (3, 5)])
def test_roi_align_degenerate_boxes_with_adaptive_sampling(out_hw):
    """sampling_ratio 0 with w = 0, h = 0, both 0 and h smaller than one bin: ceil(roi / bins) samples per bin - with none the
    output is exactly zero (the sum is divided by max(count, 1)), never NaN; otherwise it equals the helper"""
    import pool_edge_cases as P
    feat, lvl = _roi_level(torch.float32)
    got = _roi_run(lvl, P.DEGENERATE_BOXES, out_hw, 0).cpu().double().numpy()
    want = _roi_want(feat, P.DEGENERATE_BOXES, out_hw, 0)
    assert np.isfinite(got).all()
    for r, empty in enumerate(P.DEGENERATE_EMPTY):
        assert (np.abs(got[r]).max() == 0.0) == empty, P.DEGENERATE_BOXES[r]
    np.testing.assert_allclose(got, want, rtol=0, atol=ROI_TOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_roi_align_rotated_boxes_over_the_corners_into_interleaved_channels(dtype):
    """rotated boxes hanging over each corner of the map (part of the samples skipped, part clamped), fp32 and fp16 levels,
    written into every second channel of a wider output (out_coff = 1, out_cstride = 2): the written channels equal the helper
    within 1e-4, the others keep their sentinel"""
    import pool_edge_cases as P
    feat, lvl = _roi_level(dtype)
    R, (PH, PW), C = len(P.CORNER_BOXES), P.CORNER_OUT, P.ROI_C
    out = torch.full((R, PH, PW, 2 * C), -77.0, device=_dev())
    _roi_run(lvl, P.CORNER_BOXES, P.CORNER_OUT, P.CORNER_SR, out=out, out_coff=1, out_cstride=2)
    o = out.cpu()
    assert (o[..., 0::2] == -77.0).all(), "an untouched channel was written"
    want = _roi_want(feat, P.CORNER_BOXES, P.CORNER_OUT, P.CORNER_SR)
    assert np.abs(want).max() > 0.1
    np.testing.assert_allclose(o[..., 1::2].double().numpy(), want, rtol=0, atol=ROI_TOL)


def test_roi_align_level_assignment_at_the_boundaries():
    """five levels, level i constant i + 1, one sample per box at a point that is inside every level: the output names the
    level.  Boxes with sqrt(w h) exactly 56 ... 896 (square and 4:1), a few fp32 ulps and a relative 1e-3 to either side, and
    far outside both ends; the expected level is the fp32 formula of d2 assign_boxes_to_levels in numpy float32, and only
    boxes whose level survives a +-2 ulp error of log2 are used (tests/pool_edge_cases.py, checked on the CPU)."""
    import pool_edge_cases as P
    from glass_amd.ops import native as K
    dev = _dev()
    cases = P.level_cases()
    feats = [torch.full((1, 32, 32, 4), float(i + 1), device=dev) for i in range(P.LEVEL_NUM)]
    scales = [1.0 / (4 << i) for i in range(P.LEVEL_NUM)]
    boxes = torch.tensor([[64.0, 64.0, w, h, 0.0] for _, w, h, _ in cases]).to(dev)      # centre: 15.5 ... 0.5 in index space
    idx = torch.zeros((len(cases),), dtype=torch.int32, device=dev)
    y = K.roi_align_rotated(feats, scales, boxes, idx, (1, 1), 1)
    torch.cuda.synchronize()
    y = y.cpu().reshape(len(cases), 4)
    assert (y == y[:, :1]).all() and (y == y.round()).all(), "a sample of a constant level must be that constant exactly"
    got = y[:, 0].long() - 1
    want = torch.tensor([lv for *_, lv in cases])
    wrong = [(cases[i], int(got[i])) for i in torch.nonzero(got != want).flatten().tolist()]
    assert torch.equal(got, want), wrong


def test_roi_align_grid_stride_loop():
    """R PH PW C/4 = 129 * 128 * 128 just above the 256 * 32 blocks of 256 threads the launch is capped at: the tail is done
    by the grid-stride loop.  Bit-equal to the same boxes pooled in two halves (each below the cap)."""
    from glass_amd.ops import native as K
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    lvl = torch.randn((1, 32, 32, 4), generator=g).to(dev)
    R = 129
    assert R * 128 * 128 > 256 * 32 * 256 == (R - 1) * 128 * 128
    boxes = torch.rand((R, 5), generator=g) * torch.tensor([32.0, 32.0, 24.0, 24.0, 360.0]) + torch.tensor([0.0, 0.0, 2.0, 2.0, -180.0])
    boxes = boxes.contiguous().to(dev)
    idx = torch.zeros((R,), dtype=torch.int32, device=dev)
    whole = K.roi_align_rotated([lvl], [1.0], boxes, idx, (128, 128), 2)
    h = 64
    parts = [K.roi_align_rotated([lvl], [1.0], boxes[a:b].contiguous(), idx[a:b].contiguous(), (128, 128), 2) for a, b in ((0, h), (h, R))]
    torch.cuda.synchronize()
    assert torch.equal(whole, torch.cat(parts))
    assert float(whole[-1].abs().max()) > 0 and float(whole[h].abs().max()) > 0


# ================================================================================================ max pooling
def _pool_reference(x, k, s, p, dtype):
    """F.max_pool2d on the CPU; for fp16 through fp32, which is exact (the values are fp16 numbers, the maximum is one of them)"""
    return F.max_pool2d(x.to(dtype).float(), k, s, p).to(dtype)


def _pool_run(x, k, s, p, dtype):
    from glass_amd.ops import native as K
    y = K.maxpool2d_nhwc(x.to(dtype).permute(0, 2, 3, 1).contiguous().to(_dev()), k, s, p)
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2).contiguous()


POOL_WINDOWS = [((3, 3), (2, 2), (1, 1)), ((2, 2), (2, 2), (0, 0)), ((2, 1), (2, 1), (0, 0)),        # the compiled windows
                ((2, 2), (2, 2), (1, 1)),                                                            # one in-bounds tap at a corner
                ((3, 2), (2, 1), (1, 0)), ((1, 3), (1, 1), (0, 1)), ((5, 5), (3, 3), (2, 2))]        # the runtime-window kernel


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("k,s,p", POOL_WINDOWS)
def test_maxpool_propagates_nan_like_torch(k, s, p, dtype):
    """NaN, +inf and -inf inside windows, at the corners (with padding (2,2)/2/1 leaves the corner window one in-bounds tap),
    and in every tap of one window: bit-equal to F.max_pool2d (int view, so NaN is compared): a NaN tap gives NaN, a window of
    -inf gives -inf"""
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(17)
    N, C, H, W = 2, 8, 13, 11
    x = torch.randn((N, C, H, W), generator=g)
    x[0, 0, 5, 5], x[0, 1, 6, 4], x[0, 2, 3, 7] = nan, inf, -inf
    x[0, 3, 6, 6], x[0, 3, 6, 7] = nan, inf                                    # NaN beside +inf: NaN wins
    x[1, 0, 0, 0], x[1, 1, 0, 0], x[1, 2, 0, 0] = nan, inf, -inf               # the corner taps
    x[1, 0, H - 1, W - 1], x[1, 1, H - 1, 0], x[1, 2, 0, W - 1] = nan, nan, -inf
    ho, wo = 2, 2                                                              # every tap of one window
    h0, w0 = max(ho * s[0] - p[0], 0), max(wo * s[1] - p[1], 0)
    x[1, 4, h0:ho * s[0] - p[0] + k[0], w0:wo * s[1] - p[1] + k[1]] = nan
    x[1, 5, h0:ho * s[0] - p[0] + k[0], w0:wo * s[1] - p[1] + k[1]] = -inf
    x[1, 6] = -inf                                                             # a whole plane of -inf
    x[1, 7, ::2] = nan
    want = _pool_reference(x, k, s, p, dtype)
    assert torch.isnan(want).any() and (want == -inf).any() and (want == inf).any()
    got = _pool_run(x, k, s, p, dtype)
    assert got.dtype == dtype and got.shape == want.shape
    bad = torch.nonzero(_bits(got) != _bits(want))
    assert bad.numel() == 0, f"{len(bad)} outputs differ, first at {bad[:4].tolist()}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shape,k,s", [((4100, 4, 32, 2), (2, 2), (2, 2)),      # N Ho = 65600 rows > 65535: rows folded onto grid y
                                       ((1, 256, 2, 260), (2, 1), (2, 1))])     # Wo C/4 = 16640 > 64 * 256: the x grid-stride loop
def test_maxpool_grid_folds(shape, k, s, dtype):
    """the rows > 65535 and per_row > 64 * 256 folds of the launch, with NaN and -inf in the folded tail"""
    g = torch.Generator().manual_seed(19)
    x = torch.randn(shape, generator=g)
    x[-1, -1, -1, -1] = float("nan")
    x[-1, 0, -2:, -2:] = -float("inf")                       # the whole last window of channel 0
    x[0, 0, 0, 0] = float("nan")
    want = _pool_reference(x, k, s, 0, dtype)
    got = _pool_run(x, k, s, 0, dtype)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.isnan(want[-1, -1, -1, -1]) and want[-1, 0, -1, -1] == -float("inf")


# ================================================================================================ image resize / preprocess
RESIZE_CASES = [((40, 64), (20, 32), "2:1 down"), ((36, 60), (24, 40), "3:2 down"), ((48, 2000), (31, 1333), "strip, non-integer down"),
                ((25, 35), (35, 49), "7:5 up"), ((1, 37), (3, 20), "H = 1"), ((29, 1), (20, 4), "W = 1")]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("src,dst,what", RESIZE_CASES)
def test_image_resize_against_float64(src, dst, what, flip, capsys):
    """K.image_u8hwc_to_chw against a float64 restatement of F.interpolate(bilinear, align_corners=False) and against
    F.interpolate itself, with and without the channel flip.

    Bound (u = 2^-24): the source coordinate f = (dst + 0.5) * (in / out) - 0.5 is formed in fp32 from a rounded ratio, a
    rounded product and a rounded difference, so |df| <= 3 u max(f) < 3 u in; the bilinear surface of 8-bit data has slope
    <= 255 per source pixel along each axis, which turns the coordinate errors into 255 * 3 u (H_in + W_in).  The blend
    hy (hx a + lx b) + ly (hx c + lx d) has 2 rounded complements, 6 rounded products and 3 rounded sums of values <= 255:
    <= 11 u 255.  Together 255 u (3 (H_in + W_in) + 11) (0.094 for the 48 x 2000 strip, 1.7e-3 for 40 x 64).  Measured maxima
    are printed; F.interpolate computes the same coordinate in fp32 with roundings of its own, so it gets twice the bound."""
    from glass_amd.ops import native as K
    from known_answers import bilinear_resize_f64
    g = torch.Generator().manual_seed(23)
    img = torch.randint(0, 256, (src[0], src[1], 3), generator=g, dtype=torch.uint8)
    got = K.image_u8hwc_to_chw(img.to(_dev()), dst, flip_channels=flip)
    torch.cuda.synchronize()
    got = got.cpu()
    chw = img.permute(2, 0, 1).flip(0) if flip else img.permute(2, 0, 1)
    want = bilinear_resize_f64(chw.numpy(), dst)
    bound = 255.0 * U * (3 * (src[0] + src[1]) + 11)
    err = float(np.abs(got.double().numpy() - want).max())
    ref = F.interpolate(chw.float()[None], size=dst, mode="bilinear", align_corners=False)[0]
    err_t = float((got - ref).abs().max())
    _say(capsys, f"resize {what} flip={flip}: max |err| vs float64 {err:.2e}, vs F.interpolate {err_t:.2e}, bound {bound:.2e}")
    assert err <= bound and err_t <= 2 * bound


@pytest.mark.parametrize("flip", [False, True])
def test_image_identity_path_is_exact(flip):
    from glass_amd.ops import native as K
    g = torch.Generator().manual_seed(29)
    img = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8)
    got = K.image_u8hwc_to_chw(img.to(_dev()), (37, 53), flip_channels=flip).cpu()
    chw = img.permute(2, 0, 1).flip(0) if flip else img.permute(2, 0, 1)
    assert torch.equal(got, chw.float())


@pytest.mark.parametrize("short", [0, 1])
def test_preprocess_image_non_unit_std_into_a_later_slot(short):
    """(x - mean) / std with a non-unit std into slot 2 of a batch pre-filled with a sentinel; the image fills the padded size
    exactly (short = 0) or is one row and one column short (the pad row / column and the 4th channel must read zero).  One
    rounded difference and one rounded quotient: relative 2 u + u^2 of the float64 value with the fp32 mean / std."""
    from glass_amd.ops import native as K
    dev = _dev()
    g = torch.Generator().manual_seed(31)
    Hp, Wp = 32, 40
    H, W = Hp - short, Wp - short
    chw = torch.randint(0, 256, (3, H, W), generator=g).float()
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    batch = torch.full((3, Hp, Wp, 4), 7.0, device=dev)
    K.preprocess_image(chw.to(dev), mean, std, batch, 2)
    torch.cuda.synchronize()
    b = batch.cpu()
    assert (b[:2] == 7.0).all(), "another slot was written"
    m32, s32 = np.array(mean, dtype=np.float32).astype(np.float64), np.array(std, dtype=np.float32).astype(np.float64)
    want = np.zeros((Hp, Wp, 4))
    want[:H, :W, :3] = (chw.permute(1, 2, 0).double().numpy() - m32) / s32
    got = b[2].double().numpy()
    assert (got[H:] == 0).all() and (got[:, W:] == 0).all() and (got[..., 3] == 0).all()
    assert (np.abs(got - want) <= 2.5 * U * np.abs(want)).all()


# ================================================================================================ mask branch and small fry
def test_sigmoid_at_the_ends_of_the_range():
    """0 -> exactly 0.5; +inf, 104 and 88 -> exactly 1 (1 - e^-88 rounds to 1); -inf and -104 -> exactly 0 (e^-104 is below
    half the smallest subnormal); NaN -> NaN; elsewhere (-88, whose 6e-39 is a subnormal number, and ordinary values)
    rtol 1e-6 of the float64 value"""
    from glass_amd.ops import native as K
    nan, inf = float("nan"), float("inf")
    vals = [0.0, -0.0, 88.0, -88.0, 104.0, -104.0, inf, -inf, nan, 1.0, -1.0, 10.0, -10.0, 30.0, -30.0, 60.0, -60.0, 0.5, -87.0]
    reps = 27
    x = torch.tensor(vals * reps + [0.25] * 3)                      # 516 elements: not a multiple of the 256-thread block
    y = K.sigmoid_(x.to(_dev()))
    torch.cuda.synchronize()
    y = y.cpu()
    rows = _bits(y[:reps * len(vals)]).view(reps, len(vals))
    assert (rows == rows[:1]).all() and (y[-3:] == y[-3]).all()
    y = y[:len(vals)]
    exact = {0: 0.5, 1: 0.5, 2: 1.0, 4: 1.0, 5: 0.0, 6: 1.0, 7: 0.0}
    for i, v in exact.items():
        assert float(y[i]) == v, (vals[i], float(y[i]))
        assert float(torch.sigmoid(torch.tensor(vals[i]))) == v     # torch's answer too
    assert math.isnan(float(y[8]))
    for i in (3, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18):
        want = 1.0 / (1.0 + math.exp(-vals[i]))
        assert abs(float(y[i]) - want) <= 1e-6 * want, (vals[i], float(y[i]), want)


def test_paste_rotated_masks_threshold_degenerate_boxes_and_unaligned_rows():
    """W = 11 (not a multiple of 4, odd: with R > 1 most output rows start at an address that is not 4-byte aligned, so the
    byte-wise store path runs).  Box 0 is axis-aligned and as large as its 8 x 8 mask, so image pixel (y, x) reads mask
    (y, x) with weight exactly 1: values of exactly 0.5 must come out set (>=), the fp32 neighbour below 0.5 clear.  Boxes
    with w = 0, h = 0 or NaN coordinates give an all-clear mask.  A rotated box is compared with the oracle's paste."""
    from glass_amd.ops import native as K
    from oracle import glass_cpu as O
    M, H, W = 8, 9, 11
    g = torch.Generator().manual_seed(37)
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    pattern = torch.tensor([0.5, below, 0.5000001, 0.0, 1.0, 0.5, below, 0.25])
    m0 = torch.stack([pattern.roll(r) for r in range(M)])
    masks = torch.rand((6, M, M), generator=g)
    masks[0] = m0
    nan = float("nan")
    boxes = torch.tensor([[4.0, 4.0, 8.0, 8.0, 0.0], [5.0, 4.0, 0.0, 6.0, 0.0], [5.0, 4.0, 6.0, 0.0, 20.0],
                          [nan, 4.0, 6.0, 5.0, 0.0], [5.0, 4.0, 6.0, nan, 10.0], [5.5, 4.25, 9.0, 5.0, 33.0]])
    got = K.paste_rotated_masks(masks.to(_dev()), boxes.to(_dev()), (H, W), 0.5)
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == torch.bool and got.shape == (6, H, W)
    want0 = torch.zeros((H, W), dtype=torch.bool)
    want0[:M, :M] = m0 >= 0.5
    assert torch.equal(got[0], want0)
    for r in (1, 2, 3, 4):
        assert not got[r].any(), f"box {boxes[r].tolist()} must give an all-clear mask"
    ref = O.paste_rotated_masks(masks[5:], boxes[5:], (H, W), 0.5)
    assert torch.equal(got[5], ref[0].bool()) and got[5].any() and not got[5].all()


def test_pixel_shuffle_mean_over_h_and_mul_at_ragged_sizes():
    """element counts that are no multiple of the 256-thread block (and, for mul_, one above the launch's block cap):
    pixel shuffle against the exact rearrangement, mean over H (H = 1 exact, H = 8 against a float64 sum within the H
    roundings of a sequential fp32 sum plus the division), mul_ bit-equal to the fp32 product"""
    from glass_amd.ops import native as K
    dev = _dev()
    g = torch.Generator().manual_seed(41)
    N, H, W, C = 3, 5, 7, 12
    x = torch.randn((N, H, W, 4 * C), generator=g)
    assert (x.numel() // 4) % 256 != 0
    y = K.pixel_shuffle2x_nhwc(x.to(dev)).cpu()
    assert torch.equal(y, x.view(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C))
    for Hm in (1, 8):
        x = torch.randn((3, Hm, 7, 12), generator=g)
        y = K.mean_over_h(x.to(dev)).cpu()
        assert y.shape == (3, 7, 12)
        if Hm == 1:
            assert torch.equal(y, x[:, 0])
        else:
            want = x.double().mean(dim=1)
            bound = (Hm + 1) * U * x.double().abs().sum(dim=1) / Hm
            assert ((y.double() - want).abs() <= bound).all()
    for n in (3 * 7 * 5 * 4, 4 * (256 * 4096 + 3)):
        a, b = torch.randn((n,), generator=g), torch.randn((n,), generator=g)
        got = K.mul_(a.to(dev).clone(), b.to(dev)).cpu()
        assert torch.equal(got, a * b)
