"""GPU: the device ring simplifier (csrc/ring_simplify.hip through ops.native.simplify_rings and MaskPolygonizer(simplify=))
against the host statement glass_amd.evaluation.simplify_ring, vertex for vertex and offset for offset: the shared cases, the
lane-stride and staging boundaries, the 2^20 case, through both tracers, through the polygonizer with its `keep_valid`
fallback, through the writer, and on bad input."""
import io
import zipfile
from unittest import mock

import numpy as np
import pytest
import torch

import ring_simplify_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _pack(rings, dev):
    """rings -> (xy int32 [V, 2], ring_off int32 [R + 1]) on the device, the tracers' form"""
    flat = np.asarray([p for r in rings for p in r], dtype=np.int32).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    return torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)


def _unpack(xy, off):
    assert xy.dtype == off.dtype == torch.int32 and xy.dim() == 2 and xy.shape[1] == 2
    pts, off = xy.cpu().numpy().tolist(), off.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(pts)
    return [pts[a:b] for a, b in zip(off[:-1], off[1:])]


def _assert_rings(got, want, names, what):
    assert len(got) == len(want), what
    for name, g, w in zip(names, got, want):
        assert g == w, f"{what}, {name}: device ring of {len(g)} vertices, host ring of {len(w)}; first difference at " \
                       f"{next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))}"


@pytest.fixture(scope="module")
def batch():
    """(names, rings): every ring of the direct comparison, in one call, with empty rings between non-empty ones"""
    from glass_amd.ops import native as K
    cases = list(C.all_cases())
    cases += [(f"chain of {k} interior vertices", C.chain_ring(k)) for k in (63, 64, 65, 127, 128, 129)]
    limit = K.RING_SIMPLIFY_LDS_POINTS
    cases += [(f"long ring of {n} points", C.long_ring(n)) for n in (limit, limit + 1)]      # staged in LDS / read from global memory
    closed = C.long_ring(limit)
    cases += [(f"closed long ring of {limit + 1} points", closed + [closed[0]])]
    names, rings = [], []
    for k, (name, ring) in enumerate(cases):
        names.append(name)
        rings.append(ring)
        if k % 5 == 2:
            names.append(f"empty after {name}")
            rings.append([])
    assert max(len(r) for r in rings) == limit + 1 and rings[-1] != [] and [] in rings
    return names, rings


@pytest.mark.parametrize("tol", C.TOLERANCES + (1024,))
def test_equals_the_host_statement(batch, tol):
    from glass_amd.evaluation import simplify_rings_host
    from glass_amd.ops import native as K
    names, rings = batch
    xy, off = _pack(rings, _dev())
    got = _unpack(*K.simplify_rings(xy, off, tol))
    want = simplify_rings_host(rings, tol)
    _assert_rings(got, want, names, f"tolerance {tol}")
    if tol == 1024:                                                    # the decisions beyond 53 bits
        for name, ring, _, kept in C.high_bit_cases():
            assert (ring[1] in got[names.index(f"high bit, {name}")]) == kept, name
    assert tol == 0 or sum(len(g) for g in got) < sum(len(r) for r in rings)


def test_no_rings_and_no_points_launch_nothing():
    from glass_amd.ops import native as K
    dev = _dev()
    e2 = torch.empty((0, 2), dtype=torch.int32, device=dev)
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        xy, off = K.simplify_rings(e2, torch.zeros((1,), dtype=torch.int32, device=dev), 1)
        assert tuple(xy.shape) == (0, 2) and off.tolist() == [0] and xy.dtype == off.dtype == torch.int32
        xy, off = K.simplify_rings(e2, torch.zeros((4,), dtype=torch.int32, device=dev), 1)
        assert tuple(xy.shape) == (0, 2) and off.tolist() == [0, 0, 0, 0]


def test_through_both_tracers():
    import roi_mask_cases as RC
    from glass_amd.evaluation import masks_to_polygons, simplify_rings_host
    from glass_amd.ops import native as K
    dev = _dev()
    masks = C.curved_band_masks(8, 3)
    assert masks.shape == (8, 96, 128)
    got = _unpack(*K.simplify_rings(*K.mask_rings(torch.from_numpy(masks).to(dev)), 1.0))
    want = simplify_rings_host(C.traced(masks), 1.0)
    _assert_rings(got, want, range(8), "mask_rings")
    assert 3 * sum(len(g) for g in got) < sum(len(t) for t in C.traced(masks))
    for c in RC.cases():
        m, b = torch.from_numpy(c["masks"]).to(dev), torch.from_numpy(c["boxes"]).to(dev)
        got = _unpack(*K.simplify_rings(*K.roi_mask_rings(m, b, c["hw"], c["threshold"]), 1.0))
        pasted = K.paste_rotated_masks(m, b, c["hw"], c["threshold"]).cpu().numpy()
        want = simplify_rings_host([C.int_ring(r) for r in masks_to_polygons(pasted)], 1.0)
        _assert_rings(got, want, range(len(want)), c["name"])


def test_polygonizer_simplifies_and_without_the_argument_returns_what_it_did():
    import roi_mask_cases as RC
    from glass_amd.evaluation import MaskPolygonizer, masks_to_polygons, simplify_rings_host
    from glass_amd.ops import native as K
    dev = _dev()
    masks = np.concatenate([C.curved_band_masks(6, 4), np.zeros((1, 96, 128), dtype=bool), C.curved_band_masks(2, 5)])
    plain = MaskPolygonizer(dev)(masks)
    assert plain == masks_to_polygons(masks) and plain[6] == []
    assert MaskPolygonizer(dev, simplify=None, keep_valid=False)(masks) == plain
    for keep_valid in (True, False):
        got = MaskPolygonizer(dev, simplify=1.0, keep_valid=keep_valid)(masks)
        assert got == (C.host_polygons(plain, 1.0) if keep_valid else simplify_rings_host(plain, 1.0)) and got[6] == []
        assert all(isinstance(v, float) for r in got for p in r for v in p)
    c = RC.cases()[0]
    m, b = torch.from_numpy(c["masks"]).to(dev), torch.from_numpy(c["boxes"]).to(dev)
    plain = MaskPolygonizer(dev).from_rois(m, b, c["hw"], c["threshold"])
    assert plain == masks_to_polygons(K.paste_rotated_masks(m, b, c["hw"], c["threshold"]).cpu().numpy())
    assert MaskPolygonizer(dev, simplify=1.0, keep_valid=False).from_rois(m, b, c["hw"], c["threshold"]) == simplify_rings_host(plain, 1.0)
    with mock.patch.object(K, "simplify_rings", side_effect=AssertionError("simplified")):
        with mock.patch.object(K, "ring_check", side_effect=AssertionError("checked")):
            assert MaskPolygonizer(dev)(masks[:2]) == masks_to_polygons(masks[:2])       # the same launches as ever
    for bad in (0.3, -1, 2000):
        with pytest.raises(ValueError):
            MaskPolygonizer(dev, simplify=bad)


@pytest.mark.parametrize("tol", (2, 3, 4, 5, 6))
def test_keep_valid_returns_the_traced_ring_for_exactly_the_rings_simplification_breaks(tol):
    from glass_amd.evaluation import MaskPolygonizer
    case = C.invalid_after_simplification()
    dev = _dev()
    masks = torch.from_numpy(case["masks"]).to(dev)
    broken = {k for k, t in case["found"] if t == tol}
    as_float = lambda ring: [[float(x), float(y)] for x, y in ring]
    poly = MaskPolygonizer(dev, simplify=tol)
    got = poly(masks)
    want = [as_float(case["rings"][k] if k in broken else case["simplified"][tol][k]) for k in range(len(masks))]
    _assert_rings(got, want, range(len(want)), f"keep_valid, tolerance {tol}")
    assert poly.restored == len(broken)
    loose = MaskPolygonizer(dev, simplify=tol, keep_valid=False)
    _assert_rings(loose(masks), [as_float(r) for r in case["simplified"][tol]], range(len(want)), f"keep_valid=False, tolerance {tol}")
    assert loose.restored == 0
    if tol == 6:
        assert len(case["found"]) >= 3 and len({t for _, t in case["found"]}) >= 2


def _lines(det_zip):
    with zipfile.ZipFile(io.BytesIO(det_zip)) as z:
        return {n: z.read(n).decode().splitlines() for n in sorted(z.namelist())}


def test_writer_det_lines_equal_the_host_path_and_none_is_lost():
    from glass_amd.evaluation import MaskPolygonizer, RingChecker, TextResultWriter, masks_to_polygons
    from test_gpu_rrc_score import _writer_case
    dev = _dev()
    enc, inputs, outputs, gt = _writer_case("totaltext", 12, 10, True)

    host_polygons = lambda masks: C.host_polygons(masks_to_polygons(masks), 1.0)
    host = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=host_polygons)
    host.process(inputs, outputs)
    for out in outputs:                                                # as the model leaves them: on the device
        inst = out["instances"]
        if len(inst):
            inst.pred_masks = inst.pred_masks.to(dev)
    device = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=MaskPolygonizer(dev, simplify=1.0),
                              ring_checker=RingChecker(dev))
    device.process(inputs, outputs)
    unsimplified = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=MaskPolygonizer(dev), ring_checker=RingChecker(dev))
    unsimplified.process(inputs, outputs)
    assert device.coco_results() == host.coco_results()
    with mock.patch("time.time", return_value=1_700_000_000.0):
        za, zb, zc = (w.det_zip(w.to_eval_format(w.coco_results(), 0.5, 0.4)) for w in (host, device, unsimplified))
    a, b, c = _lines(za), _lines(zb), _lines(zc)
    assert a == b and za == zb
    count = lambda files: {n: len(l) for n, l in files.items()}
    assert count(b) == count(c) and sum(count(b).values()) > 10
    points = lambda files: sum(l.split(",####")[0].count(",") + 1 for ls in files.values() for l in ls) // 2
    print(f"[ring_simplify] writer: {points(c)} points in the det lines unsimplified, {points(b)} at 1 px")
    assert points(b) < points(c)


def test_bad_input_raises_and_does_not_fault():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    dev = _dev()
    ring = C.staircase(6)
    xy, off = _pack([ring, [], ring], dev)
    far = xy.clone()
    far[len(ring) + 3, 1] = (1 << 20) + 1
    with pytest.raises(GlassLibraryError, match="status 1"):
        K.simplify_rings(far, off, 1)
    far[len(ring) + 3, 1] = -(1 << 20) - 1
    with pytest.raises(GlassLibraryError, match="status 1"):
        K.simplify_rings(far, off, 1)
    far[len(ring) + 3, 1] = -(1 << 20)                                 # the bound itself is in range
    K.simplify_rings(far, off, 1)
    for bad_off in ([0, len(ring), len(ring) - 1, 2 * len(ring)], [0, len(ring), len(ring), 2 * len(ring) + 1], [-1, len(ring), len(ring), 2 * len(ring)]):
        with pytest.raises(GlassLibraryError, match="status 2"):
            K.simplify_rings(xy, torch.tensor(bad_off, dtype=torch.int32, device=dev), 1)
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        for bad_xy, bad_o in ((xy.to(torch.int64), off), (xy, off.to(torch.int64)), (xy.float(), off), (xy.cpu(), off), (xy, off.cpu()),
                              (xy.reshape(-1), off), (xy.repeat(1, 2)[:, ::2], off), (xy, off.reshape(1, -1)), (xy, off[:0])):
            with pytest.raises(GlassLibraryError):
                K.simplify_rings(bad_xy, bad_o, 1)
        for bad_tol in (0.3, -0.25, 1024.25, float("nan")):
            with pytest.raises(ValueError):
                K.simplify_rings(xy, off, bad_tol)
    got = _unpack(*K.simplify_rings(xy, off, 1))                       # and the device is as well as before
    assert got == [[[0, 0], [6, 6], [-6, 6], [0, 0]], [], [[0, 0], [6, 6], [-6, 6], [0, 0]]]


def test_two_runs_are_bit_for_bit_equal(batch):
    from glass_amd.ops import native as K
    xy, off = _pack(batch[1], _dev())
    for tol in (0.25, 1, 6):
        a, b = K.simplify_rings(xy, off, tol), K.simplify_rings(xy, off, tol)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1][-1]) == a[0].shape[0] > 0
