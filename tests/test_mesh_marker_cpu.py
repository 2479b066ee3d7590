"""The mesh marker without a device: the numpy restatement (tests/mesh_marker_ref.py) against a literal per-vertex
transcription of fillMarkerWithMesh [recalled] on a mesh with degenerate triangles, hand-worked values of every mode, the
HEIGHT scene of the GPU test shown to reach all six rainbow sectors and both clamps, and the C ABI's new symbols."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_marker_ref as R
from tests import mesh_ref as mr
from tests import separated_mesh_ref as sr
from tests.test_mesh_cpu import edge_case_layer
from voxgraph_amd import capi

F = np.float32

HEIGHT_Z_BLOCKS = (-3, 0, 3, 5, 7, 10, 12, 15)


def height_layer(seed=0, vps=8):
    """a sparse column of blocks at voxel size 0.1 (block size 0.8): z from below -1 to above 10"""
    rng = np.random.default_rng(seed)
    bi = np.array([(0, 0, z) for z in HEIGHT_Z_BLOCKS], np.int32)
    d = rng.uniform(-0.3, 0.3, (len(bi), vps ** 3)).astype(F)
    return 0.1, vps, (bi, d, np.ones_like(d))


_CACHE = {}


def edge_case_mesh():
    """(vertices, normals, rgba) of mesh_ref's mesh of the layer with the planted corner cases, a colour per triangle"""
    if "edge" not in _CACHE:
        layer = edge_case_layer(np.random.default_rng(2), 8, (-2, -1, -1), (2, 2, 2))
        _, _, v, n, _ = mr.generate_mesh(*layer, 8, 0.1)
        rgba = (np.arange(len(v))[:, None] * np.array([7, 5, 3, 1]) + np.array([0, 90, 180, 9])).astype(np.uint8)
        _CACHE["edge"] = (v, n, rgba)
    return _CACHE["edge"]


def height_mesh():
    if "height" not in _CACHE:
        vs, vps, layer = height_layer()
        _CACHE["height"] = mr.generate_mesh(*layer, vps, vs)[2:4]
    return _CACHE["height"]


def literal_marker(v, n, rgba, mode, opacity, constant_rgba=None):
    """fillMarkerWithMesh [recalled], one vertex at a time in scalars"""
    def c8(k):
        return F(float(int(k)) / 255.0)

    def unit(x, y, z):
        x, y, z = F(x), F(y), F(z)
        ln = F(np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z))))
        return [F(x / ln), F(y / ln), F(z / ln)]

    lights = (unit(0.8, -0.2, 0.7), unit(-0.5, 0.2, 0.2))
    points, colors = [], []
    for t in range(len(v)):
        for c in range(3):
            p = v[t, c]
            points.append([float(p[0]), float(p[1]), float(p[2])])
            col = constant_rgba if constant_rgba is not None else (None if rgba is None else rgba[t])
            if mode == R.GRAY:
                rgb = [F(0.5)] * 3
            elif mode == R.COLOR:
                rgb = [c8(col[a]) for a in range(3)]
            elif mode == R.NORMALS:
                rgb = [F(float(n[t, a]) * 0.5 + 0.5) for a in range(3)]
            elif mode in (R.LAMBERT, R.LAMBERT_COLOR):
                if mode == R.LAMBERT:
                    col = (127, 127, 127)
                d = []
                for L in lights:
                    dot = F(F(F(n[t, 0] * L[0]) + F(n[t, 1] * L[1])) + F(n[t, 2] * L[2]))
                    d.append(F(0) if dot < F(0) else dot)
                rgb = []
                for a in range(3):
                    ch = c8(col[a])
                    val = F(F(F(d[0] * ch) + F(d[1] * ch)) + F(0.2))
                    rgb.append(F(1) if F(1) < val else val)
            else:
                ratio = F((float(p[2]) + 1.0) / 11.0)
                ratio = F(0) if ratio < 0 else ratio
                ratio = F(1) if F(1) < ratio else ratio
                rgb = [c8(k) for k in sr.rainbow_color_map(float(ratio))[:3]]
            colors.append(rgb + [F(opacity)])
    return np.array(points, np.float64).reshape(-1, 3), np.array(colors, F).reshape(-1, 4)


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_literal_transcription(mode):
    v, n, rgba = edge_case_mesh()
    assert len(v) > 1000
    assert (np.abs(n).sum(1) == 0).any()                                # degenerate triangles kept their zero normal
    got = R.fill_marker(v, n, rgba, mode, 0.75)
    want = literal_marker(v, n, rgba, mode, 0.75)
    assert R.same(got[0], want[0]) and R.same(got[1], want[1])
    assert got[0].shape == (3 * len(v), 3) and got[1].shape == (3 * len(v), 4)
    # points: the soup, exactly; alpha: the opacity, everywhere
    assert np.array_equal(got[0].astype(F).view(np.uint32), v.reshape(-1, 3).view(np.uint32))
    assert (got[1][:, 3] == F(0.75)).all()
    # a constant colour replaces the triangles' colours
    const = np.array([12, 200, 99, 3], np.uint8)
    if mode in (R.COLOR, R.LAMBERT_COLOR):
        a = R.fill_marker(v, n, None, mode, 0.5, constant_rgba=const)
        b = literal_marker(v, n, None, mode, 0.5, constant_rgba=const)
        assert R.same(a[1], b[1]) and not R.same(a[1][:, :3], got[1][:, :3])
        with pytest.raises(ValueError):
            R.fill_marker(v, n, None, mode)
    zero = np.flatnonzero(np.abs(n).sum(1) == 0)
    if mode == R.NORMALS:
        assert (got[1][3 * zero, :3] == F(0.5)).all()
    if mode == R.LAMBERT:
        assert (got[1][3 * zero, :3] == F(0.2)).all()


def test_height_restatement_equals_literal_transcription_on_the_height_scene():
    v, n = height_mesh()
    got = R.fill_marker(v, n, None, R.HEIGHT, 1.0)
    want = literal_marker(v, n, None, R.HEIGHT, 1.0)
    assert R.same(got[0], want[0]) and R.same(got[1], want[1])


def test_height_scene_hits_all_six_sectors_and_both_clamps():
    v, _ = height_mesh()
    z = v.reshape(-1, 3)[:, 2]
    raw = ((z.astype(np.float64) + 1.0) / 11.0).astype(F)
    assert (raw < 0).sum() > 50 and (raw > 1).sum() > 50                # both clamps
    t = R.height_ratio(z)
    assert t.min() == 0 and t.max() == 1
    inside = (raw > 0) & (raw < 1)
    assert sorted(set(R.rainbow_sector(t[inside]).tolist())) == [0, 1, 2, 3, 4, 5]
    assert all((R.rainbow_sector(t[inside]) == s).sum() > 50 for s in range(6))
    assert R.rainbow_sector(np.array([1.0], F))[0] == 0                  # h - floor(h): the upper clamp is red again
    # the vectorised map is the library's and the separated mesh's
    ts = np.concatenate([t[::7], np.linspace(0, 1, 1001).astype(F)])
    want = np.array([sr.rainbow_color_map(float(x))[:3] for x in ts], np.uint8)
    assert np.array_equal(R.rainbow_bytes(ts), want)
    assert np.array_equal(want, np.array([capi.rainbow_color_map(float(x))[:3] for x in ts], np.uint8))


def _one(normal=(0, 0, 1), rgba=(255, 255, 255, 255), z=0.0):
    v = np.array([[[0, 0, z], [1, 0, z], [0, 1, z]]], F)
    return v, np.array([normal], F), np.array([rgba], np.uint8)


def test_hand_worked_values():
    v, n, c = _one()
    assert R.fill_marker(v, n, c, R.NORMALS)[1][0].tolist() == [0.5, 0.5, 1.0, 1.0]
    assert R.fill_marker(v, n, c, R.GRAY, 0.25)[1].tolist() == [[0.5, 0.5, 0.5, 0.25]] * 3
    v0, n0, c0 = _one(normal=(0, 0, 0))
    assert (R.fill_marker(v0, n0, c0, R.LAMBERT)[1][:, :3] == F(0.2)).all()
    assert (R.fill_marker(v0, n0, c0, R.NORMALS)[1][:, :3] == F(0.5)).all()
    # white at the normal L1: d1 = |L1|^2 ~ 1, d2 = max(0, L1 . L2) = 0, v ~ 1.2: clamped
    assert R.L1 @ R.L2 < 0
    vl, nl, cl = _one(normal=tuple(R.L1))
    assert (R.fill_marker(vl, nl, cl, R.LAMBERT_COLOR)[1][:, :3] == F(1)).all()
    grey = R.fill_marker(vl, nl, cl, R.LAMBERT)[1][0, 0]                 # 127 / 255 of it: below the clamp
    assert 0.69 < grey < 0.70
    assert R.fill_marker(v, n, np.array([[255, 0, 51, 7]], np.uint8), R.COLOR, 0.5)[1][0].tolist() == [1.0, 0.0, float(F(0.2)), 0.5]
    assert R.C8[255] == 1 and R.C8[0] == 0 and R.C8[127] == F(127 / 255)
    # HEIGHT: z = -1 is t = 0 (red), just below is clamped to the same, z = 10 is t = 1 (h - floor(h) = 0: red), above too
    below = np.nextafter(F(-1), F(-2))
    for z in (-1.0, below, 10.0, 11.5):
        vz, nz, cz = _one(z=z)
        assert R.fill_marker(vz, nz, cz, R.HEIGHT)[1].tolist() == [[1.0, 0.0, 0.0, 1.0]] * 3, z
    # z = 4.5: t = 0.5, sector 3, f = 0 -> (0, 255, 255)
    vz, nz, cz = _one(z=4.5)
    assert R.fill_marker(vz, nz, cz, R.HEIGHT)[1][0].tolist() == [0.0, 1.0, 1.0, 1.0]
    # per vertex, not per triangle
    vz[0, 1, 2] = 10.0
    col = R.fill_marker(vz, nz, cz, R.HEIGHT)[1]
    assert col[0].tolist() == col[2].tolist() != col[1].tolist()
    # points: f32 widened
    x = F(0.1)
    vz[0, 0, 0] = x
    assert R.fill_marker(vz, nz, cz, R.GRAY)[0][0, 0] == float(x) != 0.1
    # empty, and what the restatement refuses
    e = R.fill_marker(np.zeros((0, 3, 3), F), np.zeros((0, 3), F), None, R.LAMBERT_COLOR, constant_rgba=(1, 2, 3, 4))
    assert e[0].shape == (0, 3) and e[1].shape == (0, 4)
    for bad in (-1, 6):
        with pytest.raises(ValueError):
            R.fill_marker(v, n, c, bad)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            R.fill_marker(v, n, c, R.GRAY, bad)


def test_symbols_exported_with_the_declared_signatures_and_null_handles_refused():
    lib = capi.load()
    vp, i32p, i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    want = {
        "vgx_mesh_marker_config_default": (None, [C.POINTER(capi.MeshMarkerConfig)]),
        "vgx_mesh_marker_create": (C.c_int, [vp, C.POINTER(vp)]),
        "vgx_mesh_marker_destroy": (C.c_int, [vp]),
        "vgx_mesh_fill_marker": (C.c_int, [vp, C.POINTER(capi.MeshMarkerConfig), vp]),
        "vgx_mesh_marker_stats": (C.c_int, [vp, i64p, i32p]),
        "vgx_mesh_marker_download": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_float)]),
        "vgx_mesh_marker_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name) and capi.SIGNATURES[name] == sig, name
    assert [f[0] for f in capi.MeshMarkerConfig._fields_] == ["color_mode", "opacity", "use_constant_color", "constant_rgba"]
    assert C.sizeof(capi.MeshMarkerConfig) == 16
    assert (capi.MARKER_COLOR, capi.MARKER_HEIGHT, capi.MARKER_NORMALS, capi.MARKER_GRAY, capi.MARKER_LAMBERT,
            capi.MARKER_LAMBERT_COLOR) == R.MODES == (0, 1, 2, 3, 4, 5)
    assert hasattr(capi, "MeshMarker") and hasattr(capi, "fill_marker")
    cfg = capi.mesh_marker_config()
    assert (cfg.color_mode, cfg.opacity, cfg.use_constant_color, list(cfg.constant_rgba)) == (R.LAMBERT_COLOR, 1.0, 0, [0, 0, 0, 0])
    out = C.c_void_p(5)
    assert lib.vgx_mesh_marker_create(None, C.byref(out)) == capi.ERR_INVALID and out.value == 5
    assert lib.vgx_mesh_marker_destroy(None) == capi.ERR_INVALID
    assert lib.vgx_mesh_fill_marker(None, None, None) == capi.ERR_INVALID
    n = C.c_int64(7)
    assert lib.vgx_mesh_marker_stats(None, C.byref(n), None) == capi.ERR_INVALID and n.value == 7
    assert lib.vgx_mesh_marker_download(None, None, None) == capi.ERR_INVALID
    assert lib.vgx_mesh_marker_device_pointers(None, None, None) == capi.ERR_INVALID
