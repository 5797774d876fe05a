"""CPU: the tile plan of tiled inference (glass_amd/inference/tiling.py), the float64 reference of the cross-view merge
(tests/view_merge_cases.py) on hand-made known answers, and the per-feature header include/glass_hip_ext_views.h with its
binding - parsing, the cross-compiled library's symbols, and every limit the host side of glass_merge_views refuses."""
import ctypes
import math
import os

import numpy as np
import pytest

import view_merge_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEMMA_SETS = ((64, 32, 4), (64, 16, 8), (96, 40, 0), (32, 8, 3))       # (64, 16, 8): L = 0, the lemma's degenerate end - points only
PLAN_SETS = ((64, 32, 4), (64, 24, 8), (96, 40, 0), (32, 8, 3))        # what plan_tiles accepts: 2*border < overlap
INF = float("inf")


def _plan(*a):
    from glass_amd.inference.tiling import plan_tiles
    return plan_tiles(*a)


# ------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("tile,overlap,border", LEMMA_SETS)
def test_every_interval_up_to_L_lies_in_some_keep_interval(tile, overlap, border):
    """the coverage lemma, exhaustively: extents 1..399, every interval [a, min(a + L, extent)], L = overlap - 2*border, lies
    inside the keep interval of some tile (a shorter interval lies inside one of these).  The keep sides are integers, so
    whether a real interval fits depends only on whether its start is an integer or lies strictly between two: the starts
    k and k + 1/2 stand for all of them.  On the per-axis functions plan_tiles is made of (it refuses L = 0 itself)."""
    from glass_amd.inference.tiling import axis_keep, axis_origins
    L = overlap - 2 * border
    for extent in range(1, 400):
        size = min(tile, extent)
        keeps = [axis_keep(o, size, extent, border) for o in axis_origins(extent, tile, overlap)]
        if L > 0:
            p = _plan(extent, 1, tile, overlap, border)
            assert p.max_whole == L and [(t.keep[1], t.keep[3]) for t in p.tiles] == keeps      # along y: the axis of `extent`
        for a2 in range(2 * extent + 1):
            a = a2 / 2.0
            b = min(a + L, float(extent))
            assert any(lo <= a and b <= hi for lo, hi in keeps), (extent, a)


@pytest.mark.parametrize("tile,overlap,border", PLAN_SETS)
def test_plan_shape(tile, overlap, border):
    for extent in list(range(1, 400, 7)) + [tile - 1, tile, tile + 1, 2 * tile - overlap, 2 * tile - overlap + 1]:
        other = 2 * tile + 5
        p = _plan(extent, other, tile, overlap, border)
        assert len(p.tiles) == len(p.ys) * len(p.xs) and len(set(p.tiles)) == len(p.tiles)
        assert {(t.h, t.w) for t in p.tiles} == {(min(tile, extent), tile)}          # equal sizes
        assert [(t.y0, t.x0) for t in p.tiles] == [(y, x) for y in p.ys for x in p.xs]
        for origins, ext in ((p.ys, extent), (p.xs, other)):
            size = min(tile, ext)
            assert origins[0] == 0 and origins[-1] + size == ext                       # first at 0, last flush with the edge
            assert list(origins) == sorted(set(origins))
            for a, b in zip(origins, origins[1:]):
                assert a + size - b >= overlap                                         # consecutive tiles overlap
            if ext <= tile:
                assert origins == (0,)
        for t in p.tiles:
            kx0, ky0, kx1, ky1 = t.keep
            assert kx0 == (-INF if t.x0 == 0 else t.x0 + border) and kx1 == (INF if t.x0 + t.w == other else t.x0 + t.w - border)
            assert ky0 == (-INF if t.y0 == 0 else t.y0 + border) and ky1 == (INF if t.y0 + t.h == extent else t.y0 + t.h - border)


def test_plan_known_answer_and_refusals():
    p = _plan(160, 224, 128, 64, 8)
    assert p.ys == (0, 32) and p.xs == (0, 64, 96) and p.max_whole == 48
    assert p.tiles[4] == (32, 64, 128, 128, (72.0, 40.0, 184.0, INF))
    assert _plan(100, 90, 128, 64, 8).tiles == ((0, 0, 100, 90, (-INF, -INF, INF, INF)),)
    for bad in ((100, 100, 100, 32, 4), (100, 100, 0, 0, 0), (100, 100, 64, 64, 4), (100, 100, 64, 70, 4), (100, 100, 64, 8, 4), (100, 100, 64, 16, 8),
                (100, 100, 64, 32, -1), (100, 100, 64, 0, 0), (0, 100, 64, 32, 4)):
        with pytest.raises(ValueError):
            _plan(*bad)


# ------------------------------------------------------------------------------------------------ float64 replay, known answers
def _merge(views, xform, keep, band, thr=0.5, max_out=1024):
    """views: per view a list of (box, score)"""
    V, K = len(views), max(len(v) for v in views)
    boxes, scores = np.zeros((V, K, 5), dtype=np.float32), np.zeros((V, K), dtype=np.float32)
    for v, rows in enumerate(views):
        for s, (b, sc) in enumerate(rows):
            boxes[v, s], scores[v, s] = b, sc
    counts = np.array([len(v) for v in views], dtype=np.int32)
    return C.merge_ref(boxes, scores, counts, np.array(xform, dtype=np.float32), np.array(keep, dtype=np.float32),
                       np.array(band, dtype=np.float32), thr, max_out)


def test_reference_known_answers():
    box = (50.0, 40.0, 30.0, 10.0, 15.0)
    free = [C.ALL, C.ALL], [[-INF, INF]] * 2
    # two identical boxes in two views: one survivor, the better-scored; at equal scores the lower view
    r = _merge([[(box, 0.6)], [(box, 0.9)]], [[0, 0, 1]] * 2, *free)
    assert r["src"].tolist() == [1] and r["count"] == 1 and r["flag"] == 0
    assert _merge([[(box, 0.7)], [(box, 0.7)]], [[0, 0, 1]] * 2, *free)["src"].tolist() == [0]
    # the same boxes through different frames: view 1 is shifted by (20, 10) and at half resolution
    half = ((50.0 - 20) / 2, (40.0 - 10) / 2, 15.0, 5.0, 15.0)
    r = _merge([[(box, 0.6)], [(half, 0.9)]], [[0, 0, 1], [20, 10, 2]], *free)
    assert r["src"].tolist() == [1] and np.array_equal(r["boxes"][0], np.array(box, dtype=np.float32))
    # the same two boxes in ONE view: both stay, in score order
    r = _merge([[(box, 0.6), (box, 0.9)], []], [[0, 0, 1]] * 2, *free)
    assert r["src"].tolist() == [1, 0]
    # a fragment that touches the tile's interior edge (x = 128, keep side 120) is dropped; the same fragment at an image edge stays
    frag = (118.0, 40.0, 20.0, 10.0, 0.0)                              # x from 108 to 128
    assert _merge([[(frag, 0.9)]], [[0, 0, 1]], [[-INF, -INF, 120.0, INF]], [[-INF, INF]])["count"] == 0
    assert _merge([[(frag, 0.9)]], [[0, 0, 1]], [[-INF, -INF, INF, INF]], [[-INF, INF]])["src"].tolist() == [0]
    inside = (108.0, 40.0, 20.0, 10.0, 0.0)                            # x from 98 to 118
    assert _merge([[(inside, 0.9)]], [[0, 0, 1]], [[-INF, -INF, 120.0, INF]], [[-INF, INF]])["count"] == 1
    # a word of size L + 1 is whole in the tile and in the full view (half resolution): only the full view's copy counts
    L = 48.0
    big = (70.0, 60.0, L + 1, 12.0, 0.0)
    big_half = (35.0, 30.0, (L + 1) / 2, 6.0, 0.0)
    small = (70.0, 90.0, L - 1, 12.0, 0.0)
    small_half = (35.0, 45.0, (L - 1) / 2, 6.0, 0.0)
    r = _merge([[(big, 0.9), (small, 0.8)], [(big_half, 0.5), (small_half, 0.95)]], [[0, 0, 1], [0, 0, 2]], [C.ALL, C.ALL],
               [[-INF, L], [L, INF]])
    assert r["src"].tolist() == [1, 2]                                 # small from the tile (slot 1), big from the full view
    # the cap: three far-apart words, max_out 2 -> flag 1; max_out 3 -> flag 0
    far = [[((50.0 + 100 * i, 40.0, 30.0, 10.0, 0.0), 0.9 - 0.1 * i) for i in range(3)]]
    r = _merge(far, [[0, 0, 1]], [C.ALL], [[-INF, INF]], max_out=2)
    assert r["src"].tolist() == [0, 1] and r["flag"] == 1
    assert _merge(far, [[0, 0, 1]], [C.ALL], [[-INF, INF]], max_out=3)["flag"] == 0


def test_frame_replay_rounds_every_operation():
    """cx * inv + ox with the product rounded to float32 first - not a fused multiply-add"""
    b = np.array([1.0 + 2.0 ** -23, 0.0, 1.0, 1.0, 0.0], dtype=np.float32)
    inv, ox = np.float32(1.0 + 2.0 ** -23), np.float32(-1.0)
    got = C.frame_f32(b, (ox, 0.0, inv))[0]
    assert got == np.float32(np.float32(b[0] * inv) + ox)
    assert float(got) != float(b[0]) * float(inv) + float(ox)          # (what one rounding at the end would give)


def test_cases_hold_their_margins_and_properties():
    for case in (C.one_view_identity(), C.two_views_duplicates(), C.same_view_pairs(), C.grid_3x3_plus_full(),
                 C.counts_edges(), C.nonfinite_and_empty()) + tuple(C.chunks(*t) for t in C.CHUNK_TOTALS):
        assert C.margin_violations(case) == []
    assert C.margin_violations(C.ties(), ties=True) == []
    r = C.one_view_identity()["ref"]
    assert r["src"].tolist() == list(range(37))
    c = C.two_views_duplicates()
    assert c["ref"]["count"] == c["words"] == 40 and c["ref"]["candidates"] == 80
    c = C.same_view_pairs()
    assert c["ref"]["count"] == c["ref"]["candidates"] == 2 * c["pairs"] + 10
    c = C.grid_3x3_plus_full()
    r = c["ref"]
    views = r["src"] // c["K"]
    assert set(views.tolist()) == set(range(10))                       # every tile and the full view contribute
    assert c["rows"]["fragment"] > 0 and r["count"] < r["candidates"] < int(c["counts"].sum())
    angles = c["boxes"].reshape(-1, 5)[r["src"], 4]
    for a in C.GRID_ANGLES:                                            # the special angles, within the jitter
        assert (np.abs(angles - a) <= 1.5).any(), a
    # the known structure: every word is found exactly once
    for kind, w in c["words"]:
        hits = [i for i in range(r["count"]) if math.hypot(r["boxes"][i, 0] - w[0], r["boxes"][i, 1] - w[1]) < 3.0
                and abs(r["boxes"][i, 2] - w[2]) < 0.1 * w[2]]
        assert len(hits) == 1, (kind, w, hits)
        assert (views[hits[0]] == 9) == (kind == "large"), (kind, w)
    t = C.ties()["ref"]
    order = list(zip(t["scores"].tolist(), (t["src"] // 24).tolist(), (t["src"] % 24).tolist()))
    assert order == sorted(order, key=lambda x: (-x[0], x[1], x[2])) and t["count"] == 30


# ------------------------------------------------------------------------------------------------ header and binding
NAMES = ["glass_merge_views_workspace_bytes", "glass_merge_views"]


def test_views_header_and_binding():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", "glass_hip_ext_views.h")) as fh:
        text = fh.read()
    assert '#include "glass_hip.h"' in text
    sigs = _lib.signatures(text)
    assert list(sigs) == NAMES == _lib.ADDON_EXPORTS == list(_lib.addon_signatures())
    assert [os.path.basename(p) for p in _lib.addon_headers()] == ["glass_hip_ext_views.h"]
    assert _lib.EXT_EXPORTS == ["glass_beam_search_lexicon_workspace_bytes", "glass_beam_search_lexicon"]
    assert len(_lib.EXPORTS) == 105 and not set(NAMES) & set(_lib.EXPORTS + _lib.EXT_EXPORTS)
    for other in ("glass_hip.h", "glass_hip_ext.h"):
        with open(os.path.join(ROOT, "include", other)) as fh:
            assert "glass_merge_views" not in fh.read()
    _lib.build_library()
    L = _lib.lib()
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.glass_merge_views_workspace_bytes.restype is l and L.glass_merge_views_workspace_bytes.argtypes == [i, i]
    assert L.glass_merge_views.restype is i
    assert L.glass_merge_views.argtypes == [p] * 6 + [i, i, f, i] + [p] * 4 + [p, l, p]
    assert L.glass_abi_version() == _lib.ABI_VERSION == 8
    assert L.glass_merge_views_workspace_bytes(41, 100) >= 41 * 100 * 5 * 4          # at least the global boxes
    assert L.glass_merge_views_workspace_bytes(8, 1024) <= 1 << 20 and L.glass_merge_views_workspace_bytes(0, 1) > 0


def test_a_name_declared_twice_is_refused(tmp_path, monkeypatch):
    from glass_amd import _lib
    inc = tmp_path / "include"
    inc.mkdir()
    for name in ("glass_hip.h", "glass_hip_ext.h", "glass_hip_ext_views.h"):
        with open(os.path.join(ROOT, "include", name)) as fh:
            (inc / name).write_text(fh.read())
    (inc / "glass_hip_ext_zz.h").write_text('#include "glass_hip.h"\nint glass_merge_views_workspace_bytes(int V);\n')
    monkeypatch.setattr(_lib, "INCLUDE", str(inc))
    monkeypatch.setattr(_lib, "_ADDON_SIGNATURES", None)
    with pytest.raises(_lib.GlassLibraryError, match="glass_merge_views_workspace_bytes"):
        _lib.addon_signatures()
    (inc / "glass_hip_ext_zz.h").write_text('#include "glass_hip.h"\nint glass_zz_probe(int V, float* out);\n')
    monkeypatch.setattr(_lib, "_ADDON_SIGNATURES", None)
    assert list(_lib.addon_signatures()) == NAMES + ["glass_zz_probe"]             # sorted header order
    monkeypatch.setattr(_lib, "_ADDON_SIGNATURES", None)


def test_every_limit_is_refused_on_the_host():
    """no device needed: every refusal comes before the first runtime call.  The pointers are never dereferenced."""
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a = (a + 15) // 16 * 16
    big = 1 << 30

    def call(V=2, K=8, thr=0.5, max_out=16, ins=(a,) * 6, outs=(a,) * 4, ws=a, ws_bytes=big):
        return L.glass_merge_views(*ins, V, K, thr, max_out, *outs, ws, ws_bytes, None)

    bad = [dict(V=-1), dict(V=257, K=1), dict(K=0), dict(K=1025, V=1), dict(V=9, K=1024), dict(V=256, K=33), dict(max_out=0),
           dict(max_out=1025), dict(thr=float("nan")), dict(thr=float("inf")), dict(ws=None), dict(ws=a + 4), dict(ws_bytes=8),
           dict(ws_bytes=int(L.glass_merge_views_workspace_bytes(2, 8)) - 1)]
    bad += [dict(outs=tuple(None if j == k else a for j in range(4))) for k in range(4)]
    bad += [dict(ins=tuple(None if j == k else a for j in range(6))) for k in range(6)]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0, kw
        msg = L.glass_last_error().decode()
        assert msg.startswith("glass_merge_views"), (kw, msg)
    for V, K in ((-1, 8), (257, 1), (2, 0), (2, 1025), (9, 1024)):
        assert L.glass_merge_views_workspace_bytes(V, K) < 0
        assert L.glass_last_error().decode().startswith("glass_merge_views_workspace_bytes")
