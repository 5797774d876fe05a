"""Every conv route on EXACT operands (tests/conv_exact_cases.py): the float64 answer bit for bit, with poisoned strides.

Each tensor operand of a row (x, residual, out) is a view into the middle of a larger flat allocation with a guard band on
either side (the view starts on a 16-byte boundary).  The guards, the input channels at and beyond Cin and the residual
channels at and beyond Cout hold NaN, the whole output allocation holds one recognisable NaN bit pattern.  A row then demands:
the path the table names; the written window equal to the expected array BIT FOR BIT (compared as integers: -0.0 and NaN cannot
hide) - on the F(4x4) rows, which cannot be exact (case module), within the project's bound of the output range against the
exact reference and identical between two launches; every output finite (a NaN means the kernel read what it must not); every
bit outside the window - the other channels of the output pixels, the output's guards, and the whole input / residual
allocations - unchanged; N = 0 rows return and touch nothing.  No row hands a kernel a descriptor its predicate refuses
(tests/test_conv_exact_cases.py pins that on the host); a refused row runs the fallback it names, to the same standard."""
import collections

import numpy as np
import pytest
import torch

import conv_exact_cases as CE

pytestmark = pytest.mark.gpu

GUARD = 64                                     # elements before and behind every view: 256 / 128 bytes, views stay 16-byte aligned
PATTERN = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.float16: (torch.int16, 0x7E5A)}      # quiet NaNs with a payload
NP_OF = {torch.float32: np.float32, torch.float16: np.float16}
F43_RATIOS = collections.defaultdict(float)    # route -> largest error / bound of its F(4x4) rows


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Guarded:
    """one operand inside its own flat allocation: `flat` [GUARD | numel | GUARD] on the device, `t` the operand"""

    def __init__(self, shape, dtype, values=None):
        n = int(np.prod(shape))
        if values is None:                     # an output: the NaN pattern everywhere
            idt, pat = PATTERN[dtype]
            host = torch.full((GUARD + n + GUARD,), pat, dtype=idt).view(dtype)
        else:                                  # an input: NaN guards around the (NaN-padded) values
            host = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype)
            host[GUARD:GUARD + n] = torch.from_numpy(np.array(values, dtype=NP_OF[dtype]).reshape(-1))
        self.dtype, self.shape, self.n = dtype, tuple(shape), n
        self.before = host.view(PATTERN[dtype][0]).clone()
        self.flat = host.to(_dev())
        self.t = self.flat[GUARD:GUARD + n].view(self.shape)
        assert n == 0 or self.t.data_ptr() % 16 == 0

    def bits(self):
        return self.flat.cpu().view(PATTERN[self.dtype][0])

    def assert_untouched(self, what):
        assert torch.equal(self.bits(), self.before), f"{what}: the kernel wrote into an allocation it only reads"


def _dense(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(_dev())


def _check_output(case, out, ref, tag=""):
    """assertions 2-5 on a guarded output `out` [N,Ho,Wo,ldy] whose window must hold `ref` [N,Ho,Wo,Cout] (float64, exact)"""
    idt = PATTERN[out.dtype][0]
    npdt = NP_OF[out.dtype]
    got = out.bits()
    win = slice(case.y_coff, case.y_coff + (case.Cout - 1) * case.y_cstride + 1, case.y_cstride)
    body = got[GUARD:GUARD + out.n].view(out.shape)
    got_win = body[..., win].clone()
    vals = got_win.view(out.dtype)
    assert bool(torch.isfinite(vals).all()), f"{tag}non-finite outputs: the kernel read poison (or left pixels unwritten)"
    want = torch.from_numpy(ref.astype(npdt))
    if case.exact:
        assert torch.equal(got_win, want.view(idt)), (
            f"{tag}{int((got_win != want.view(idt)).sum())} of {want.numel()} outputs differ from the exact result; "
            f"largest |difference| {float((vals.double() - want.double()).abs().max()):.3e}")
    else:
        scale = float(np.abs(ref).max())
        err = float((vals.double() - torch.from_numpy(ref)).abs().max()) / scale
        F43_RATIOS[case.route] = max(F43_RATIOS[case.route], err / case.bound)
        if not tag:
            print(f"{case.id}: F(4x4) error {err:.3e} of the output range, bound {case.bound:.0e}, ratio {err / case.bound:.3f}")
        assert err <= case.bound, (err, case.bound)
    # everything else holds the pattern still: the other channels of the pixels and both guards
    expect = out.before.clone()
    expect[GUARD:GUARD + out.n].view(out.shape)[..., win] = got_win
    assert torch.equal(got, expect), f"{tag}bits outside the output window changed"
    return got_win


def _run_conv(case, ops, x, res, out):
    from glass_amd.ops import native as K
    w = _dense(ops["w"])
    bias = _dense(ops["bias"]) if ops["bias"] is not None else None
    rt = CE.routing_of(case)
    with CE.forced_slices(case):
        if case.fn == "linear":
            K.linear(x.t.view(case.N, case.Cin), w.view(case.Cout, case.Cin), bias, relu=case.relu,
                     out=out.t.view(case.N, case.ldy), routing=rt)
        else:
            K.conv2d_nhwc(x.t, w, bias, stride=case.stride, padding=case.pad, relu=case.relu,
                          residual=None if res is None else res.t, res_mode=case.res_mode, out=out.t, out_coff=case.y_coff,
                          out_cstride=case.y_cstride, cin=case.Cin, winograd=case.forced, routing=rt, f43k=case.f43k)
    assert K.last_conv_path() == case.path, (K.last_conv_path(), case.path)
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def _report_f43_ratios():
    yield
    for route, ratio in sorted(F43_RATIOS.items()):
        print(f"\nF(4x4) largest error / bound on {route}: {ratio:.3f}", end="")
    print()


CONV_IDS = [c.id for c in CE.CASES if c.fn in ("conv", "linear")]


@pytest.mark.parametrize("cid", CONV_IDS)
def test_conv_route_returns_the_exact_result(cid):
    case = CE.BY_ID[cid]
    ops = CE.operands(case)
    xd, od, rd = CE.dtypes_of(case)
    Ho, Wo = case.out_hw
    x = Guarded((case.N, case.H, case.W, case.ldx), xd, ops["x"])
    res = Guarded((case.N, *case.res_hw, case.ldr), rd, ops["res"]) if case.res_mode else None
    out = Guarded((case.N, Ho, Wo, case.ldy), od)
    _run_conv(case, ops, x, res, out)
    x.assert_untouched("x")
    if res is not None:
        res.assert_untouched("residual")
    if case.N == 0:
        assert torch.equal(out.bits(), out.before), "an empty batch wrote to the output allocation"
        return
    first = _check_output(case, out, CE.conv_ref(case))
    if not case.exact:                          # not exact, but the same bits every time
        again = Guarded((case.N, Ho, Wo, case.ldy), od)
        _run_conv(case, ops, x, res, again)
        assert torch.equal(_check_output(case, again, CE.conv_ref(case), "second launch: "), first), "two launches differ"


def _bits_equal(y, ref, what):
    """an output the wrapper allocated itself (dense fp32): finite and the exact result bit for bit"""
    y = y.cpu()
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.dtype, tuple(y.shape), ref.shape)
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite outputs"
    want = torch.from_numpy(ref.astype(np.float32))
    assert torch.equal(y.view(torch.int32), want.view(torch.int32)), (
        f"{what}: {int((y.view(torch.int32) != want.view(torch.int32)).sum())} of {want.numel()} outputs differ from the exact result")


@pytest.mark.parametrize("cid", [c.id for c in CE.CASES if c.fn == "dual"])
def test_dual_source_split_returns_the_exact_result(cid):
    from glass_amd.ops import native as K
    case = CE.BY_ID[cid]
    ops = CE.operands(case)
    Ho, Wo = case.out_hw
    x1 = Guarded((case.N, case.H, case.W, case.Cin), torch.float32, ops["x"])
    x2 = Guarded((case.N, Ho, Wo, case.Cin2), torch.float32, ops["x2"])
    w = _dense(ops["w"])
    cw = K.prepare_dual_weights(w[..., :case.Cin].contiguous(), w[..., case.Cin:].contiguous())
    assert cw is not None, "the raw-tensor default routing has no exact split kernel (GLASS_PW_SPLIT / GLASS_CONV_PRECISION set?)"
    y = K.conv1x1_dual_nhwc(x1.t, x2.t, cw, _dense(ops["bias"]) if ops["bias"] is not None else None,
                            stride=case.stride[0], relu=case.relu)
    assert K.last_conv_path() == case.path
    torch.cuda.synchronize()
    _bits_equal(y, CE.conv_ref(case), case.id)
    x1.assert_untouched("x1")
    x2.assert_untouched("x2")


@pytest.mark.parametrize("cid", [c.id for c in CE.CASES if c.fn in ("backbone_stem", "local_stem")])
def test_fused_stem_returns_the_exact_result(cid):
    """the fused stems (and, on the shapes their predicates refuse, the separate launches that take the layer instead)"""
    from glass_amd.ops import native as K
    case = CE.BY_ID[cid]
    ops = CE.stem_operands(case)
    x = Guarded((case.N, case.H, case.W, 4), torch.float32, ops["x"])
    direct = dict(winograd=False, routing=K.Routing(**CE.BASE_ROUTING).replace(splitk=False), relu=1)
    if case.fn == "backbone_stem":
        w, b = _dense(ops["w"]), _dense(ops["bias"])
        assert K.backbone_stem_supported(x.t, w) == case.accepts
        if case.accepts:
            y = K.backbone_stem_fused(x.t, w, b)
        else:
            y = K.maxpool2d_nhwc(K.conv2d_nhwc(x.t, w, b, stride=2, padding=3, **direct), 3, 2, 1)
        assert K.last_conv_path() == case.path
    else:
        w1, b1, w2, b2 = (_dense(ops[k]) for k in ("w1", "b1", "w2", "b2"))
        assert K.local_stem_supported(x.t, w1, w2) == case.accepts
        if case.accepts:
            y = K.local_stem_fused(x.t, w1, b1, w2, b2)
        else:
            y = K.conv2d_nhwc(K.conv2d_nhwc(x.t, w1, b1, padding=1, **direct), w2, b2, padding=1, **direct)
            assert K.last_conv_path() == case.path
            y = K.maxpool2d_nhwc(y, 2, 2)
    torch.cuda.synchronize()
    _bits_equal(y, CE.stem_ref(case), case.id)
    x.assert_untouched("x")


# the wrappers return on an empty batch before any library call (an empty tensor has no device address); the library entries
# themselves, handed valid pointers and an N = 0 descriptor, must return success and touch nothing
EMPTY_ENTRIES = [("direct-128x32-n0", ()), ("f16-n0", ()), ("f22-64-n0", ()), ("f43-wide-n0", ()), ("pw-cin32-n0", ()),
                 ("pws-cin32-n0", (9,)), ("h16-flags7-n0", (7,)), ("h16p-64-flags7-n0", (7,)), ("f43k-full-n0", "workspace")]


@pytest.mark.parametrize("cid,extra", EMPTY_ENTRIES)
def test_library_entry_returns_on_an_empty_descriptor(cid, extra):
    import ctypes
    from glass_amd._lib import lib
    from glass_amd.ops import native as K
    case = CE.BY_ID[cid]
    assert case.N == 0
    buf = Guarded((256,), torch.float32)              # one valid, 16-byte aligned address for every pointer argument
    p = buf.t.data_ptr()
    d = CE.desc_of(case)
    tail = (2, 0, p, 1024) if extra == "workspace" else extra
    rc = getattr(lib(), case.entry)(ctypes.byref(d), p, p, p, p if case.res_mode else None, p, *tail, K.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0, (case.entry, rc, lib().glass_last_error())
    buf.assert_untouched(case.entry)
