"""CPU: the float64 reference of the fused-view merge (tests/view_fuse_cases.py) on hand-derived answers, the view plan
(glass_amd/inference/view_fusion.py) against data.transforms.RotationTransform, the margins of every seeded case, and the
feature header include/glass_hip_feature_fuse.h with its binding - parsing, the cross-compiled library's symbols, and every
argument the host side of glass_fuse_views refuses."""
import ctypes
import math
import os

import numpy as np
import pytest

import view_fuse_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = ["glass_fuse_views_workspace_bytes", "glass_fuse_views"]
HEADER = "glass_hip_feature_fuse.h"


def _plan(*a, **k):
    from glass_amd.inference.view_fusion import plan_views
    return plan_views(*a, **k)


# ------------------------------------------------------------------------------------------------ float64 replay, known answers
def _fuse(views, affine=None, bounds=C.FREE, thr=0.5, text=None, stop=1, mode=0, min_votes=1, max_out=1024):
    """views: per view a list of (box, score); text: per view a list of (arg row, max row)"""
    V, K = len(views), max(max(len(v) for v in views), 1)
    boxes, scores = np.zeros((V, K, 5), dtype=np.float32), np.zeros((V, K), dtype=np.float32)
    for v, rows in enumerate(views):
        for s, (b, sc) in enumerate(rows):
            boxes[v, s], scores[v, s] = b, sc
    arg = mx = None
    if text is not None:
        T = len(text[0][0][0])
        arg, mx = np.zeros((V, K, T), dtype=np.int32), np.ones((V, K, T), dtype=np.float32)
        for v, rows in enumerate(text):
            for s, (a, m) in enumerate(rows):
                arg[v, s], mx[v, s] = a, m
    counts = np.array([len(v) for v in views], dtype=np.int32)
    aff = np.array([C.IDENTITY] * V if affine is None else affine, dtype=np.float64)
    return C.fuse_ref(boxes, scores, counts, aff, np.array(bounds, dtype=np.float32), thr, arg, mx, stop, mode, min_votes, max_out)


BOX = (50.0, 40.0, 30.0, 10.0, 15.0)


def test_reference_two_views_one_row_two_votes():
    r = _fuse([[(BOX, 0.6)], [(BOX, 0.9)]])
    assert r["src"].tolist() == [1] and r["votes"].tolist() == [2] and r["views"].tolist() == [0b11]
    assert (r["count"], r["flag"], r["kept"], r["candidates"]) == (1, 0, 1, 2)
    assert r["scores"].tolist() == [np.float32(0.9)] and r["keys"].tolist() == [np.float32(0.9)]
    # at equal keys the lower view is kept
    assert _fuse([[(BOX, 0.7)], [(BOX, 0.7)]])["src"].tolist() == [0]
    assert _fuse([[(BOX, -0.0)], [(BOX, 0.0)]])["src"].tolist() == [0]              # -0.0 and +0.0 are one key


def test_reference_pairs_of_one_view_and_the_earliest_kept():
    """two overlapping boxes of one view both survive with one vote each; a box of a third view over both supports the
    earlier one only"""
    near = (51.0, 40.5, 30.0, 10.0, 15.0)
    r = _fuse([[(BOX, 0.9), (near, 0.8)], [], [(BOX, 0.3)]])
    assert r["src"].tolist() == [0, 1] and r["votes"].tolist() == [2, 1] and r["views"].tolist() == [0b101, 0b001]
    r = _fuse([[(BOX, 0.8), (near, 0.9)], [], [(BOX, 0.3)]])                        # the order decides, not the slot
    assert r["src"].tolist() == [1, 0] and r["votes"].tolist() == [2, 1]
    # min_votes = 2 drops the single-view rows and compacts the rest
    far = (200.0, 40.0, 30.0, 10.0, 0.0)
    views = [[(far, 0.95), (BOX, 0.9), (near, 0.8)], [], [(BOX, 0.3)]]
    r = _fuse(views, min_votes=2)
    assert r["src"].tolist() == [1] and r["votes"].tolist() == [2] and (r["count"], r["kept"], r["flag"]) == (1, 3, 0)
    assert _fuse(views, min_votes=3)["count"] == 0
    # n > max_out after the vote filter: flag 1 although the walk was not cut
    r = _fuse(views, max_out=2)
    assert r["src"].tolist() == [0, 1] and (r["count"], r["flag"], r["cut"], r["kept"]) == (2, 1, 0, 3)


def test_reference_rank_modes_and_word_score():
    """the copy that reads best wins in modes 1 and 2; the word score stops at, and includes, the stop symbol"""
    stop = 1
    good, bad = ([5, 6, stop, 9], [0.9, 0.8, 0.5, 0.001]), ([5, 6, 7, 8], [0.9, 0.1, 0.9, 0.9])
    views, text = [[(BOX, 0.9)], [(BOX, 0.6)]], [[bad], [good]]
    assert _fuse(views, text=text, mode=0)["src"].tolist() == [0]
    for mode in (1, 2):
        r = _fuse(views, text=text, mode=mode)
        assert r["src"].tolist() == [1] and r["votes"].tolist() == [2]
        ws = np.float32(np.float32(np.float32(0.9) * np.float32(0.8)) * np.float32(0.5))
        assert r["keys"][0] == (np.float32(np.float32(0.6) * ws) if mode == 1 else ws) and r["scores"][0] == np.float32(0.6)
    assert C.word_score_f32(*bad, stop) == np.float32(np.float32(np.float32(np.float32(0.9) * np.float32(0.1)) * np.float32(0.9)) * np.float32(0.9))
    assert C.word_score_f32([stop, 3], [0.25, 0.5], stop) == np.float32(0.25)
    # a key that is not finite is no candidate
    r = _fuse(views, text=[[([5, 6, 7, 8], [0.9, np.nan, 0.9, 0.9])], [good]], mode=2)
    assert r["src"].tolist() == [1] and r["votes"].tolist() == [1] and r["candidates"] == 1


def test_reference_bounds_are_closed_and_one_ulp_outside_is_dropped():
    case = C.on_the_bounds()
    r = case["ref"]
    kept = sorted(r["src"].tolist())
    assert kept == [i for i, inside in enumerate(case["inside"]) if inside]
    assert _fuse([[(BOX, 0.9)]], bounds=(-INF, -INF, 50.0, INF))["count"] == 1
    assert _fuse([[(BOX, 0.9)]], bounds=(-INF, -INF, np.nextafter(np.float32(50.0), np.float32(0.0)), INF))["count"] == 0
    assert _fuse([[(BOX, 0.9)]], bounds=(-INF, 40.0, INF, 40.0))["count"] == 1
    assert _fuse([[(BOX, 0.9)]], bounds=(np.nan, -INF, INF, INF))["count"] == 0


def test_reference_the_180_degree_view_sees_the_same_word():
    """a box at angle a in the 0-degree view, and the same word as the 180-degree view sees it (the forward map of
    RotationTransform), come back to IoU 1 and merge; the angles wrap into [-180, 180)"""
    from glass_amd.data.transforms import RotationTransform
    H, W = 120, 200
    views = _plan(H, W, (0.0, 180.0, 90.0), (1.0,), lambda hw: 1.0)
    box = np.array([60.0, 40.0, 30.0, 10.0, 25.0], dtype=np.float32)
    seen = [v.rotation.apply_rotated_boxes(box[None])[0] for v in views]
    assert seen[1].tolist() == [W - 60.0, H - 40.0, 30.0, 10.0, -155.0]
    r = _fuse([[(seen[0], 0.5)], [(seen[1], 0.9)], [(seen[2], 0.7)]], affine=[v.affine for v in views])
    assert r["src"].tolist() == [1] and r["votes"].tolist() == [3] and r["views"].tolist() == [0b111]
    assert r["boxes"][0].tolist() == box.tolist()
    # wrap: 170 + 30 -> -160; -170 - 30 -> 160; -180 stays, 180 -> -180
    for a, d, want in ((170.0, 30.0, -160.0), (-170.0, -30.0, 160.0), (-180.0, 0.0, -180.0), (180.0, 0.0, -180.0), (10.0, 710.0, 0.0)):
        got = C.frame_f64((0, 0, 1, 1, a), (1, 0, 0, 0, 1, 0, 1, d))[4]
        assert got == np.float32(want) and -180.0 <= got < 180.0, (a, d, got)
    # the scale: w and h times s, the centre through the matrix
    g = C.frame_f64((10.0, 20.0, 8.0, 4.0, 0.0), (2.0, 0.0, 1.0, 0.0, 2.0, 3.0, 2.0, 0.0))
    assert g.tolist() == [21.0, 43.0, 16.0, 8.0, 0.0]
    t = RotationTransform(H, W, 180.0)
    assert views[1].rotation.matrix == t.matrix


def test_frame_replay_rounds_once():
    """float64 throughout, one rounding to float32 at the end - not the float32 arithmetic of glass_merge_views"""
    b = np.array([1.0 + 2.0 ** -23, 0.0, 1.0, 1.0, 0.0], dtype=np.float32)
    m0 = 1.0 + 2.0 ** -12          # the product is 1 + 2^-12 + 2^-23 + 2^-35: float32 drops the last term, float64 keeps it
    got = C.frame_f64(b, (m0, 0.0, -1.0, 0.0, 1.0, 0.0, 1.0, 0.0))[0]
    assert got == np.float32(float(b[0]) * m0 - 1.0)
    assert got != np.float32(np.float32(b[0] * np.float32(m0)) + np.float32(-1.0))


# ------------------------------------------------------------------------------------------------ the plan
PLAN_ANGLES = (0.0, 90.0, 180.0, 270.0, 30.0, -17.5, 333.0, 451.0)


@pytest.mark.parametrize("ratio", [1.0, 0.8, 1.7])
def test_plan_rows_agree_with_the_rotation_transform(ratio):
    H, W = 97, 141
    scales = (1.0, 0.5, 2.0)
    views = _plan(H, W, PLAN_ANGLES, scales, lambda hw: ratio)
    assert [(v.angle, v.scale) for v in views] == [(a, s) for a in PLAN_ANGLES for s in scales]      # angle-major, scale-minor
    g = np.random.default_rng(0)
    pts = g.uniform(-20, 200, (50, 2))
    boxes = np.concatenate([g.uniform(0, 140, (50, 2)), g.uniform(4, 40, (50, 2)), g.uniform(-180, 180, (50, 1))], 1)
    for v in views:
        t, rho, m = v.rotation, v.rho, v.affine
        assert rho == v.scale * ratio and len(m) == 8
        assert (t.h, t.w) == (H, W) and t.angle == v.angle % 360.0
        # points of the view: divided by rho they are points of the rotated image
        mapped = np.stack([m[0] * pts[:, 0] + m[1] * pts[:, 1] + m[2], m[3] * pts[:, 0] + m[4] * pts[:, 1] + m[5]], 1)
        assert np.abs(mapped - t.inverse_coords(pts / rho)).max() <= 1e-9
        # boxes of the view (float64 all the way): centre and size divided by rho are boxes of the rotated image
        in_rot = boxes.copy()
        in_rot[:, :4] /= rho
        want = t.inverse_rotated_boxes(in_rot)
        got = np.stack([m[0] * boxes[:, 0] + m[1] * boxes[:, 1] + m[2], m[3] * boxes[:, 0] + m[4] * boxes[:, 1] + m[5],
                        boxes[:, 2] * m[6], boxes[:, 3] * m[6], boxes[:, 4] + m[7]], 1)
        got[:, 4] = got[:, 4] - 360.0 * np.floor((got[:, 4] + 180.0) / 360.0)
        assert np.abs(got[:, :4] - want[:, :4]).max() <= 1e-9
        d = np.abs(got[:, 4] - want[:, 4])
        assert np.minimum(d, 360.0 - d).max() <= 1e-9
        # there and back: a box of the image, forward-mapped and scaled by rho, comes back to itself
        fwd = t.apply_rotated_boxes(boxes)
        fwd[:, :4] *= rho
        back = np.stack([m[0] * fwd[:, 0] + m[1] * fwd[:, 1] + m[2], m[3] * fwd[:, 0] + m[4] * fwd[:, 1] + m[5],
                         fwd[:, 2] * m[6], fwd[:, 3] * m[6], fwd[:, 4] + m[7]], 1)
        back[:, 4] = back[:, 4] - 360.0 * np.floor((back[:, 4] + 180.0) / 360.0)
        assert np.abs(back[:, :4] - boxes[:, :4]).max() <= 1e-6
        d = np.abs(back[:, 4] - boxes[:, 4])
        assert np.minimum(d, 360.0 - d).max() <= 1e-6
        # and view_fuse_cases' forward map is the inverse of the row
        assert np.abs(C.to_view(boxes[0], m)[:4] - fwd[0, :4]).max() <= 1e-6


def test_plan_ratio_callback_and_known_rows():
    seen = []
    views = _plan(100, 60, (0.0, 90.0), (1.0, 2.0), lambda hw: seen.append(tuple(hw)) or (0.5 if hw[0] == 100 else 0.25))
    assert seen == [(100, 60), (60, 100)]                               # the rotated image's (height, width), once per angle
    assert [v.rho for v in views] == [0.5, 1.0, 0.25, 0.5]
    assert views[0].affine == (2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 2.0, -0.0)
    assert views[1].affine[:7] == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0)
    assert views[2].affine == (0.0, -4.0, 60.0, 4.0, 0.0, 0.0, 4.0, -90.0)       # out[i, j] = in[j, w - 1 - i]
    assert views[0].rotation is views[1].rotation and views[2].rotation.out_hw == (60, 100)


def test_plan_refusals():
    one = lambda hw: 1.0
    bad = [dict(angles=(), scales=(1.0,)), dict(angles=(0.0,), scales=()), dict(angles=(0.0, INF), scales=(1.0,)),
           dict(angles=(float("nan"),), scales=(1.0,)), dict(angles=(0.0,), scales=(1.0, INF)), dict(angles=(0.0,), scales=(0.0,)),
           dict(angles=(0.0,), scales=(-1.0,)), dict(angles=(0.0, 360.0), scales=(1.0,)), dict(angles=(10.0, -350.0), scales=(1.0,)),
           dict(angles=(0.0,), scales=(1.0, 1.0)), dict(angles=tuple(range(65)), scales=(1.0,)),
           dict(angles=tuple(range(13)), scales=(1.0, 2.0, 3.0, 4.0, 5.0)), dict(angles=5.0, scales=(1.0,))]
    for kw in bad:
        with pytest.raises(ValueError, match="plan_views"):
            _plan(50, 60, ratio_of=one, **kw)
    assert len(_plan(50, 60, tuple(range(64)), (1.0,), one)) == 64
    assert len(_plan(50, 60, tuple(range(16)), (1.0, 2.0, 3.0, 4.0), one)) == 64
    with pytest.raises(ValueError, match="ratio_of"):
        _plan(50, 60, (0.0,), (1.0,), lambda hw: 0.0)


# ------------------------------------------------------------------------------------------------ the seeded cases
def test_cases_hold_their_margins_and_properties():
    redrawn = 0
    for make in C.ALL_CASES + (C.keep_exact, C.keep_cut) + tuple((lambda t=t: C.chunks(*t)) for t in C.CHUNK_TOTALS):
        case = make()
        assert C.margin_violations(case, ranks=case["ranks"]) == []
        redrawn += case["redrawn"]
    assert C.margin_violations(C.ties(), ties=True) == [] and C.margin_violations(C.on_the_bounds(), on_bound=True) == []
    print(f"[view_fuse_cases] rows redrawn over all builders: {redrawn}; rejected seeds: 0")
    assert C.one_view_identity()["ref"]["src"].tolist() == list(range(37))
    # the scene: every word comes out once, with the views that hold it
    c = C.scene_four_rotations()
    assert int(c["counts"].sum()) == sum(len(h) for h in c["held"]) + c["outside"]
    differ = 0
    for rank in ("detection", "product", "word"):
        for mv in (1, 2, 3, 4):
            r = C.ref_of(c, rank, mv)
            want = [h for h in c["held"] if len(h) >= mv]
            assert r["count"] == len(want) and r["kept"] == len(c["held"]) and r["flag"] == 0, (rank, mv)
            assert sorted(r["views"].tolist()) == sorted(sum(1 << v for v in h) for h in want), (rank, mv)
            assert (r["votes"] >= mv).all() and (r["src"] // c["K"] < 4).all()
    det, wrd = C.ref_of(c, "detection"), C.ref_of(c, "word")
    by_mask = lambda r: {(round(float(b[0])) // 24, round(float(b[1])) // 24): s for b, s in zip(r["boxes"], r["src"])}
    a, b = by_mask(det), by_mask(wrd)
    differ = sum(1 for k in a if k in b and a[k] != b[k])
    assert differ >= 8, differ                                           # the best-detected and the best-read copy differ
    t = C.ties()["ref"]
    order = list(zip(t["keys"].tolist(), (t["src"] // 24).tolist(), (t["src"] % 24).tolist()))
    assert order == sorted(order, key=lambda x: (-x[0], x[1], x[2])) and t["count"] == 30
    assert sorted(t["votes"].tolist()) == [1] * 24 + [2] * 6
    c = C.same_view_pairs()
    r = c["ref"]
    assert r["count"] == 2 * c["pairs"] + 10 and r["candidates"] == 3 * c["pairs"] + 10
    v0 = [(int(s), int(n), int(m)) for s, n, m in zip(r["src"], r["votes"], r["views"]) if s // c["K"] == 0]
    assert sorted(v0) == sorted([(2 * i, 2, 0b101) for i in range(c["pairs"])] + [(2 * i + 1, 1, 0b001) for i in range(c["pairs"])])


# ------------------------------------------------------------------------------------------------ header and binding
def test_fuse_header_and_binding():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", HEADER)) as fh:
        text = fh.read()
    assert '#include "glass_hip.h"' in text
    sigs = _lib.signatures(text)
    assert list(sigs) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    assert HEADER in [os.path.basename(p) for p in _lib.feature_headers()]
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER:
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_fuse_views" not in fh.read(), other
    _lib.build_library()
    L = _lib.lib()
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.glass_fuse_views_workspace_bytes.restype is l and L.glass_fuse_views_workspace_bytes.argtypes == [i, i]
    assert L.glass_fuse_views.restype is i
    assert L.glass_fuse_views.argtypes == [p] * 5 + [i, i, i] + [p, p] + [i, i, f, i, i] + [p] * 7 + [p, l, p]
    assert sigs["glass_fuse_views"] == (i, L.glass_fuse_views.argtypes)
    assert L.glass_abi_version() == _lib.ABI_VERSION
    assert L.glass_fuse_views_workspace_bytes(41, 100) >= 41 * 100 * 6 * 4           # at least the boxes and the keys
    assert L.glass_fuse_views_workspace_bytes(8, 1024) <= 1 << 20 and L.glass_fuse_views_workspace_bytes(0, 1) > 0
    assert L.glass_fuse_views_workspace_bytes(64, 128) > 0
    from glass_amd.ops import native as K
    assert (K.FUSE_VIEWS_MAX_VIEWS, K.FUSE_VIEWS_MAX_SLOTS, K.FUSE_VIEWS_MAX_OUT) == (64, 8192, 1024)


def test_every_refused_argument_returns_its_code():
    """no device needed: every refusal comes before the first runtime call.  The pointers are never dereferenced."""
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    big = 1 << 30

    def call(V=2, K=8, T=4, stop=1, mode=1, thr=0.5, min_votes=1, max_out=16, ins=(a,) * 3, text=(a, a), frames=(a, a), outs=(a,) * 7,
             ws=a, ws_bytes=big):
        return L.glass_fuse_views(*ins, *text, T, stop, mode, *frames, V, K, thr, min_votes, max_out, *outs, ws, ws_bytes, None)

    bad = [dict(V=-1), dict(V=65, K=1), dict(K=0), dict(K=1025, V=1), dict(V=9, K=1024), dict(V=64, K=129), dict(max_out=0),
           dict(max_out=1025), dict(min_votes=0), dict(min_votes=65), dict(min_votes=-1), dict(mode=-1), dict(mode=3), dict(stop=-1),
           dict(T=0), dict(T=65), dict(T=-3, mode=2), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=-float("inf")),
           dict(ws=None), dict(ws=a + 4), dict(ws_bytes=8), dict(ws_bytes=int(L.glass_fuse_views_workspace_bytes(2, 8)) - 1),
           dict(text=(None, a)), dict(text=(a, None)), dict(text=(None, None), mode=2), dict(frames=(None, a)), dict(frames=(a, None))]
    bad += [dict(outs=tuple(None if j == k else a for j in range(7))) for k in range(7)]
    bad += [dict(ins=tuple(None if j == k else a for j in range(3))) for k in range(3)]
    bad += [dict(V=0, max_out=0), dict(V=0, outs=(a,) * 6 + (None,)), dict(V=0, min_votes=0)]        # V == 0 is checked all the same
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, (kw, rc)                                        # GLASS_EINVAL
        msg = L.glass_last_error().decode()
        assert msg.startswith("glass_fuse_views"), (kw, msg)
    for V, K in ((-1, 8), (65, 1), (2, 0), (2, 1025), (9, 1024)):
        assert L.glass_fuse_views_workspace_bytes(V, K) == -1
        assert L.glass_last_error().decode().startswith("glass_fuse_views_workspace_bytes")
