"""The case table of tests/conv_exact_cases.py checked without a GPU: its float64 reference against torch, the exactness
premises of its operands (budgets, fp16 round trips, a second order of summation), and every row's accept / refuse flag and
expected path against the library's host-only *_supported() predicates and ops.native.plan_conv."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as CE

IDS = [c.id for c in CE.CASES]
CONV_FNS = ("conv", "linear", "dual")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from glass_amd import _lib
    _lib.build_library()


def _torch_conv(case, dtype):
    """the dense-equivalent problem with torch's CPU convolution in `dtype`: y = act(conv(x, w) + bias [+ residual])"""
    ops = CE.operands(case)
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    nchw = lambda a: t(a).permute(0, 3, 1, 2)
    w = ops["w"]
    y = F.conv2d(nchw(ops["x"][..., :case.Cin]), nchw(w[..., :case.Cin]), None, stride=case.stride, padding=case.pad)
    if case.Cin2:
        y = y + F.conv2d(nchw(ops["x2"]), nchw(w[..., case.Cin:]), None)
    if ops["bias"] is not None:
        y = y + t(ops["bias"]).view(1, -1, 1, 1)
    if case.relu == 2:
        y = F.relu(y)
    if case.res_mode:
        r = nchw(ops["res"][..., :case.Cout])
        y = y + (F.interpolate(r, scale_factor=2, mode="nearest") if case.res_mode == 2 else r)
    if case.relu == 1:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).numpy()


def _torch_stem(case, dtype):
    ops = CE.stem_operands(case)
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    nchw = lambda a: t(a).permute(0, 3, 1, 2)
    if case.fn == "backbone_stem":
        y = F.relu(F.conv2d(nchw(ops["x"][..., :3]), nchw(ops["w"][..., :3]), t(ops["bias"]), stride=2, padding=3))
        y = F.max_pool2d(y, 3, 2, 1)
    else:
        y = F.relu(F.conv2d(nchw(ops["x"]), nchw(ops["w1"]), t(ops["b1"]), padding=1))
        y = F.max_pool2d(F.relu(F.conv2d(y, nchw(ops["w2"]), t(ops["b2"]), padding=1)), 2, 2)
    return y.permute(0, 2, 3, 1).numpy()


def _torch_ref(case, dtype):
    return _torch_conv(case, dtype) if case.fn in CONV_FNS else _torch_stem(case, dtype)


def test_every_route_keeps_its_rows():
    counts = collections.Counter(c.route for c in CE.CASES)
    assert dict(counts) == CE.ROUTE_ROWS
    assert len(CE.CASES) == sum(CE.ROUTE_ROWS.values())


@pytest.mark.parametrize("cid", IDS)
def test_reference_and_premises(cid):
    case = CE.BY_ID[cid]
    ref = CE.conv_ref(case)
    Ho, Wo = case.out_hw
    if case.fn in CONV_FNS:
        assert ref.shape == (case.N, Ho, Wo, case.Cout)
    # the reference restates the operator: torch's float64 convolution of the dense-equivalent problem, exactly
    assert np.array_equal(ref, _torch_ref(case, torch.float64))
    # exactness budget (the transformed-domain one on the F(2x2) rows)
    b = CE.budget(case)
    assert b < CE.BUDGET_LIMIT, b
    if CE.is_f22(case):
        bt = CE.budget_f22(case)
        assert bt < CE.BUDGET_LIMIT, bt
        if case.N:        # ... and the algorithm the budget speaks about IS the convolution: At [sum U . V] A in float64, no rounding
            assert np.array_equal(CE.f22_apply(case), CE._taps(case, CE.operands(case)["x"][..., :case.Cin], CE.operands(case)["w"]))
    # the expected fp32 output is the exact value
    assert np.isfinite(ref).all()
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    # a second, independent order of summation: torch's fp32 CPU convolution returns the same bits
    got32 = _torch_ref(case, torch.float32)
    assert got32.dtype == np.float32 and np.array_equal(got32.view(np.int32), ref.astype(np.float32).view(np.int32))
    # every operand is an fp16 number (the fp16 routes see the same values), NaN poison aside
    ops = CE.operands(case) if case.fn in CONV_FNS else CE.stem_operands(case)
    for name, v in ops.items():
        if v is None:
            continue
        f = v[np.isfinite(v)]
        assert np.array_equal(f.astype(np.float16).astype(np.float64), f), name
    if case.fn in CONV_FNS and case.wide and case.N:
        # wide rows: operands that are more than one bf16 piece (the middle pieces of the split carry bits)
        bf16 = lambda v: torch.from_numpy(np.array(v, dtype=np.float32)).bfloat16().double().numpy()
        for name in ("x", "w") if case.wide == 9 else ("x",):
            f = ops[name][np.isfinite(ops[name])]
            # (|a| >= 256 and odd needs the ninth bit: a quarter of the draws, less the quarter of x forced to zero)
            assert (bf16(f) != f).mean() > 0.15, name
    if case.fn in CONV_FNS:
        # the poison sits exactly in the channels the contract leaves unread
        assert np.isfinite(ops["x"][..., :case.Cin]).all() and np.isnan(ops["x"][..., case.Cin:]).all()
        if case.res_mode:
            assert np.isfinite(ops["res"][..., :case.Cout]).all() and np.isnan(ops["res"][..., case.Cout:]).all()
        # ReLU rows: the ReLU changes results, and its position matters where both positions are possible
        if case.relu and case.N:
            assert not np.array_equal(ref, CE.conv_ref(CE.dataclasses.replace(case, relu=0))), "the ReLU is idle"
            if case.res_mode:
                assert not np.array_equal(ref, CE.conv_ref(CE.dataclasses.replace(case, relu=3 - case.relu))), "the ReLU's position does not matter"


@pytest.mark.parametrize("cid", IDS)
def test_flags_and_paths_agree_with_the_library(cid):
    """accept / refuse against the row's predicate, and the path plan_conv gives under the row's forcing; a disagreement fails"""
    from glass_amd.ops import native as K
    case = CE.BY_ID[cid]
    verdict = CE.predicate_of(case)
    if verdict is not None:
        assert verdict == case.accepts, f"{case.predicate} says {verdict}, the row says {case.accepts}"
    # (a refused row without a predicate is refused by plan_conv itself - dense rows for the strip forms, nothing to cast -
    #  and the plan below shows it)
    if case.fn in ("conv", "linear"):
        plan = CE.plan_of(case)
        assert (plan.path, plan.entry, bool(plan.strip)) == (case.path, case.entry, case.strip)
        if case.entry in (CE.DK, CE.W43K):
            want = case.slices if case.entry == CE.DK else (case.f43k[0] if isinstance(case.f43k, tuple) else case.f43k)
            assert plan.splits == want
        if case.entry in (CE.H16, CE.H16P):
            flags = case.half & (7 if case.res_mode else 3)          # (no residual, no residual dtype)
            assert plan.flags == (flags if flags else 1) and plan.cast == (case.entry == CE.H16P and not case.half & 1)
        if case.refused_forced is not None:
            assert not case.accepts
            with pytest.raises(K.GlassLibraryError):
                CE.plan_of(case, forced=case.refused_forced)
    elif case.fn == "dual":
        assert case.accepts and (case.path, case.entry) == ("pointwise_split", CE.DUAL)
    else:
        assert (case.path, case.entry) == ((("fused_stem", CE.BSTEM) if case.fn == "backbone_stem" else ("local_stem", CE.LSTEM))
                                           if case.accepts else ("direct", CE.D))
    # the descriptor itself is valid for the entry that runs: windows inside the pixel, strides cover the channels
    assert case.y_coff + (case.Cout - 1) * case.y_cstride < case.ldy and case.ldx >= case.Cin and (not case.res_mode or case.ldr >= case.Cout)
    if case.res_mode == 2:
        assert case.out_hw[0] % 2 == 0 and case.out_hw[1] % 2 == 0
