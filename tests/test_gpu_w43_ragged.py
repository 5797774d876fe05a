"""glass_conv3x3_winograd43_ragged_nhwc: maps of width 4 k + 1 in ONE launch of the F(4x4,3x3) kernel - the full tile columns
followed by paired strip tiles that compute the last pixel column of two images each (csrc/winograd43.hip).  Checked against
torch CPU fp64 at the tolerance tests/test_gpu_f_ops.py holds this kernel to (2e-5 of the output range), bit for bit against the
body-only entry on the columns both compute, and for stores outside the output window."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

RAGGED, BODY = "glass_conv3x3_winograd43_ragged_nhwc", "glass_conv3x3_winograd43_body_nhwc"
SENTINEL = 7.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _launch(entry, x, u, bias, res, out, Cin, Cout, coff, relu):
    """the library entry itself (no routing in between): x [N,H,W,Cin], out [N,H,W,ld] written at channels [coff, coff + Cout)"""
    from glass_amd.ops import native as K
    N, H, W, ldx = x.shape
    d = K.ConvDesc(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, H, W, ldx, out.shape[3], coff, 1, relu, 1 if res is not None else 0,
                   res.shape[3] if res is not None else 0)
    p = ctypes.c_void_p
    K.check(getattr(K.lib(), entry)(ctypes.byref(d), p(x.data_ptr()), p(u.data_ptr()), p(bias.data_ptr()),
                                    p(res.data_ptr() if res is not None else None), p(out.data_ptr()),
                                    p(torch.cuda.current_stream().cuda_stream)), entry)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [5, 9, 33])
@pytest.mark.parametrize("Cin,Cout", [(32, 128), (16, 64)], ids=["wide", "narrow"])
def test_ragged_entry_geometry_sweep(Cin, Cout, W):
    """N in {1, 2, 3} (odd N: the last strip tile has no second image), H in {4, 5, 16} (ragged tile rows, top and bottom padding
    inside strip tiles), with and without a residual (res_mode 1, its own row stride), ReLU 0 / 1 / 2, bias, into a channel window
    of a sentinel-filled buffer that is itself the first N images of a buffer of N + 1:
      * every output within 2e-5 of the output range of torch CPU fp64;
      * columns 0 .. W-2 bit-identical to the body-only entry on the same inputs;
      * every sentinel outside the window and the whole image N unchanged (a stray store of a strip tile's output columns 1, 2, or
        of column 3 without a second image, lands there or on a body column);
      * a second run of the same launch bit-identical."""
    from glass_amd.ops import native as K
    dev = _dev()
    coff, ld, ldr = 4, Cout + 12, Cout + 4
    w = _rand((Cout, Cin, 3, 3), 32, (2.0 / (Cin * 9)) ** 0.5)
    b = _rand((Cout,), 33, 0.1)
    u = K.winograd_pack(w.permute(0, 2, 3, 1).contiguous().to(dev), True)
    bd = b.to(dev)
    worst = 0.0
    for N, H in itertools.product((1, 2, 3), (4, 5, 16)):
        x = _rand((N, Cin, H, W), 31 + 10 * N + H)
        res = _rand((N, Cout, H, W), 34 + 10 * N + H)
        conv = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
        rd = torch.full((N, H, W, ldr), 3.0, device=dev)
        rd[..., :Cout] = res.permute(0, 2, 3, 1).to(dev)
        for use_res, relu in itertools.product((False, True), (0, 1, 2)):
            ref = F.relu(conv) if relu == 2 else conv
            if use_res:
                ref = ref + res.double()
            if relu == 1:
                ref = F.relu(ref)
            bufs = []
            for entry in (RAGGED, BODY, RAGGED):
                big = torch.full((N + 1, H, W, ld), SENTINEL, device=dev)
                _launch(entry, xd, u, bd, rd if use_res else None, big[:N], Cin, Cout, coff, relu)
                bufs.append(big)
            torch.cuda.synchronize()
            rag, body, again = (t.cpu() for t in bufs)
            what = f"[{N},{H},{W},{Cin}]->{Cout} res={use_res} relu={relu}"
            assert torch.equal(rag, again), f"{what}: two runs differ"
            assert torch.equal(rag[N], torch.full((H, W, ld), SENTINEL)), f"{what}: image N was written"
            assert bool((rag[:N, :, :, :coff] == SENTINEL).all()) and bool((rag[:N, :, :, coff + Cout:] == SENTINEL).all()), \
                f"{what}: channels outside the window were written"
            assert torch.equal(rag[:N, :, :W - 1], body[:N, :, :W - 1]), f"{what}: body columns differ from the body-only entry"
            assert bool((body[:N, :, W - 1] == SENTINEL).all())      # (the body-only entry leaves the last column alone)
            got = rag[:N, :, :, coff:coff + Cout].permute(0, 3, 1, 2).double()
            scale = float(ref.abs().max())
            e_body = float((got[..., :W - 1] - ref[..., :W - 1]).abs().max()) / scale
            e_last = float((got[..., W - 1] - ref[..., W - 1]).abs().max()) / scale
            worst = max(worst, e_body, e_last)
            assert e_body <= 2e-5 and e_last <= 2e-5, f"{what}: max err / range = {e_body:.2e} (tile columns), {e_last:.2e} (last column)"
    print(f"F(4x4,3x3) ragged launch W={W} {Cin}->{Cout}: worst max err / range = {worst:.2e}")


@pytest.mark.gpu
def test_ragged_launch_is_what_conv2d_nhwc_takes_for_the_local_shape():
    """the product route: conv2d_nhwc on a 16 x 33 map of a layer prepared once (several workgroups, an odd RoI count) launches
    the ragged entry - path 'winograd43r', nothing packed at launch - and matches torch CPU fp64 on every column"""
    from glass_amd.ops import native as K
    dev = _dev()
    R, H, W, Cin, Cout = 5, 16, 33, 64, 128
    x, w, b = _rand((R, Cin, H, W), 41), _rand((Cout, Cin, 3, 3), 42, (2.0 / (Cin * 9)) ** 0.5), _rand((Cout,), 43, 0.1)
    res = _rand((R, Cout, H, W), 44)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1) + res.double())
    cw = K.prepare_conv_weights(w.permute(0, 2, 3, 1).contiguous().to(dev), ragged=True)
    n0 = K.packs_on_the_fly()
    y = K.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(dev), cw, b.to(dev), padding=1, relu=1,
                      residual=res.permute(0, 2, 3, 1).contiguous().to(dev), res_mode=1, winograd="f43")
    assert K.last_conv_path() == "winograd43r" and K.packs_on_the_fly() == n0
    err = float((y.cpu().permute(0, 3, 1, 2).double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-5, f"max err / range = {err:.2e}"


def _plan(N, H, W, Cin, Cout, rt=None, packs="model", res=False, **kw):
    from glass_amd.ops import native as K
    r = K.Routing(precision="fp32", winograd=True, f43=True, pw=True, h16=True, ragged="tiles", splitk=True, small_grid=True, split=9)
    r = r.replace(**(rt or {}))
    if packs == "model":
        packs = K.pack_kinds(Cout, 3, 3, Cin, "fp32", 1, ragged=True, split=r.split, strip=K.needs_strip_pack(r))
    d = K.ConvDesc(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, H, W, Cin, Cout, 0, 1, 1, 1 if res else 0, Cout if res else 0)
    f32 = torch.float32
    return K.plan_conv(d, r, x_dtype=f32, out_dtype=f32, res_dtype=f32 if res else None, res_mode=1 if res else 0, packs=packs, **kw)


def test_plan_conv_routes_width_4k_plus_1_to_the_ragged_entry():
    """host arithmetic and host-only library queries (no device): the local extractor's [256,16,33,256] layers take the ragged
    entry with no strip convolution and keep the path name bench.py's meter knows; the split-K body form keeps its strip; a load
    whose routing cannot reach the strip packs no strip weights - and the layer still takes the ragged entry"""
    from glass_amd import _lib
    from glass_amd.ops import native as K
    _lib.build_library()
    for res in (False, True):
        p = _plan(256, 16, 33, 256, 256, res=res)
        assert (p.path, p.entry, p.pack, p.splits, p.strip) == ("winograd43r", RAGGED, True, 0, False)
    p = _plan(256, 16, 33, 128, 256)                                   # layer3.0 conv1
    assert (p.path, p.entry, p.strip) == ("winograd43r", RAGGED, False)
    p = _plan(32, 16, 33, 256, 256, f43k=(4, True))                    # split-K on the full tile columns: body + strip, as before
    assert (p.path, p.entry, p.pack, p.splits, p.strip) == ("winograd43k", "glass_conv3x3_winograd43_splitk_nhwc", True, 4, True)
    p = _plan(256, 16, 33, 256, 256, rt=dict(ragged=False))            # ragged routing off: a whole extra tile column
    assert (p.path, p.entry, p.strip) == ("winograd43", "glass_conv3x3_winograd43_nhwc", False)
    for two_launches in (True, "strip"):                               # the round-4 form stays selectable: body launch + strip launch
        p = _plan(256, 16, 33, 256, 256, rt=dict(ragged=two_launches))
        assert (p.path, p.entry, p.pack, p.strip) == ("winograd43r", "glass_conv3x3_winograd43_body_nhwc", True, True)
    assert K.Routing(precision="fp32", ragged=None).ragged in ("tiles", True, False)      # (the environment decides)
    assert K.Routing(precision="fp32", ragged="tiles").ragged == "tiles" and K.Routing(precision="fp32", ragged=1).ragged is True
    p = _plan(256, 16, 33, 256, 256, rt=dict(ragged=0))
    assert (p.path, p.entry, p.strip) == ("winograd43", "glass_conv3x3_winograd43_nhwc", False)
    p = _plan(256, 16, 32, 256, 256)                                   # width 4 k: nothing ragged about it
    assert (p.path, p.entry, p.strip) == ("winograd43", "glass_conv3x3_winograd43_nhwc", False)
    # the strip pack is built only where a launch can still ask for it (the small-grid rules: F(2x2) body and split-K body forms)
    T = K.Routing(precision="fp32", winograd=True, ragged="tiles", small_grid=True)
    assert K.needs_strip_pack(T) and not K.needs_strip_pack(T.replace(small_grid=False))
    assert K.needs_strip_pack(T.replace(small_grid=False, ragged=True)) and not K.needs_strip_pack(T.replace(ragged=False))
    assert "col1" in K.pack_kinds(256, 3, 3, 256, "fp32", 1, ragged=True)
    assert K.pack_kinds(256, 3, 3, 256, "fp32", 1, ragged=True, strip=False) == [False, True]
    p = _plan(256, 16, 33, 256, 256, rt=dict(small_grid=False))
    assert (p.path, p.entry, p.pack, p.strip) == ("winograd43r", RAGGED, True, False)


def test_ragged_supported_wants_width_4k_plus_1_and_room_for_one_more_image():
    from glass_amd import _lib
    from glass_amd.ops import native as K
    _lib.build_library()
    L = K.lib()

    def ok(N, H, W, Cin=256, Cout=256, ldr=0):
        d = K.ConvDesc(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, H, W, Cin, Cout, 0, 1, 0, 1 if ldr else 0, ldr)
        return bool(L.glass_winograd43_ragged_supported(ctypes.byref(d))), bool(L.glass_winograd43_supported(ctypes.byref(d)))

    assert ok(256, 16, 33) == (True, True) and ok(1, 4, 5, 16, 64) == (True, True) and ok(3, 16, 33, ldr=256) == (True, True)
    assert ok(256, 16, 32) == (False, True) and ok(256, 16, 35) == (False, True) and ok(2, 4, 1) == (False, True)
    # 16 x 33 x 256 floats = 528 KiB per image: 1985 images are within 1 GiB, 1986 with the one the strip tiles' offsets reach are not
    assert ok(1985, 16, 33) == (False, True) and ok(1984, 16, 33) == (True, True)
    assert ok(100, 16, 33, Cin=40) == (False, False)                   # not a layer the F(4x4) kernel takes at all
