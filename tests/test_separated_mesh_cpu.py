"""The separated mesh without a device: the numpy restatement (tests/separated_mesh_ref.py) on hand-built cases, voxblox's
rainbowColorMap at hand-worked points and against the library's Python copy, and the C ABI's new symbols."""
import ctypes as C
import math

import numpy as np

from tests import mesh_ref as mr
from tests import projected_map_ref as pm
from tests import separated_mesh_ref as sr
from tests.test_mesh_cpu import sphere_layer
from voxgraph_amd import capi

F = np.float32
RED, BLUE = np.array([255, 0, 0, 255], np.uint8), np.array([0, 0, 255, 255], np.uint8)


def _two_spheres():
    """two submaps of one sphere each, vps 8: their block boxes overlap in part"""
    a = sphere_layer((0.3, 0.2, 0.1), 0.7, 8, 0.1)
    b = sphere_layer((1.1, 0.2, 0.1), 0.5, 8, 0.1)
    return a, b


def test_shared_blocks_concatenate_in_array_order():
    a, b = _two_spheres()
    Ta = np.array([1, 0, 0, 0, 0, 0, 0], F)
    Tb = np.array([math.cos(0.2), 0, 0, math.sin(0.2), 0.5, -0.25, 0.125], F)
    bi, first, v, n, rgba = sr.separated_mesh([a, b], [Ta, Tb], [RED, BLUE], 8, 0.1)
    ma = mr.generate_mesh(*a, 8, 0.1)
    mb = sr.pose_mesh(mr.generate_mesh(*b, 8, 0.1), Tb)
    rows_a = {tuple(x): k for k, x in enumerate(ma[0].tolist())}
    rows_b = {tuple(x): k for k, x in enumerate(mb[0].tolist())}
    # every block of either submap, once, ascending
    keys = [tuple(x) for x in bi.tolist()]
    assert keys == sorted(set(rows_a) | set(rows_b)) and len(keys) == len(set(keys))
    shared = [k for k in keys if k in rows_a and k in rows_b]
    only_a = [k for k in keys if k in rows_a and k not in rows_b]
    only_b = [k for k in keys if k in rows_b and k not in rows_a]
    assert shared and only_a and only_b
    n_shared_both = 0
    for j, key in enumerate(keys):
        got_v = v[first[j]:first[j + 1]]
        got_c = rgba[first[j]:first[j + 1]]
        want_v, want_c = [], []
        if key in rows_a:
            k = rows_a[key]
            want_v.append(ma[2][ma[1][k]:ma[1][k + 1]])          # (identity pose: a's own triangles)
            want_c += [RED] * int(ma[1][k + 1] - ma[1][k])
        if key in rows_b:
            k = rows_b[key]
            want_v.append(mb[2][mb[1][k]:mb[1][k + 1]])
            want_c += [BLUE] * int(mb[1][k + 1] - mb[1][k])
        want_v = np.concatenate(want_v)
        assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), key
        assert np.array_equal(got_c, np.array(want_c, np.uint8).reshape(-1, 4)), key
        if key in shared and ma[1][rows_a[key] + 1] > ma[1][rows_a[key]] and mb[1][rows_b[key] + 1] > mb[1][rows_b[key]]:
            n_shared_both += 1
            # a's triangles first (red), then b's (blue)
            assert (got_c[0] == RED).all() and (got_c[-1] == BLUE).all()
    assert n_shared_both > 0
    # swapping the array order swaps the order within shared blocks, not the blocks
    bi2, first2, v2, _, rgba2 = sr.separated_mesh([b, a], [Tb, Ta], [BLUE, RED], 8, 0.1)
    assert np.array_equal(bi2, bi) and np.array_equal(first2, first)
    assert not np.array_equal(rgba2, rgba)


def test_empty_meshes_keep_their_blocks():
    vps = 8
    bi = np.array([(0, 0, 0), (3, -1, 2), (-2, 0, 0)], np.int32)
    d = np.full((3, vps ** 3), 0.2, F)                       # no surface: every block meshes to nothing
    w = np.ones_like(d)
    bi2 = np.array([(3, -1, 2), (5, 5, 5)], np.int32)
    d2 = np.full((2, vps ** 3), -0.2, F)
    w2 = np.zeros_like(d2)                                   # nothing valid
    T = np.array([1, 0, 0, 0, 1, 2, 3], F)
    out = sr.separated_mesh([(bi, d, w), (bi2, d2, w2)], [T, T], [RED, BLUE], vps, 0.1)
    assert out[0].tolist() == [[-2, 0, 0], [0, 0, 0], [3, -1, 2], [5, 5, 5]]
    assert out[1].tolist() == [0, 0, 0, 0, 0] and len(out[2]) == len(out[3]) == len(out[4]) == 0
    # no submaps at all
    out = sr.separated_mesh([], [], [], vps, 0.1)
    assert out[0].shape == (0, 3) and out[1].tolist() == [0] and out[4].shape == (0, 4)


def test_transform_is_the_projected_map_rule_and_normals_are_not_renormalised():
    a, _ = _two_spheres()
    T = np.array([0.5, 0.5, -0.5, 0.5, 0.3, -0.7, 1.1], F)   # a general rotation
    m = mr.generate_mesh(*a, 8, 0.1)
    bi, first, v, n = sr.pose_mesh(m, T)
    assert np.array_equal(bi, m[0]) and np.array_equal(first, m[1])
    want_v = pm.transform(T[:4], T[4:], m[2].reshape(-1, 3)).reshape(-1, 3, 3)
    assert np.array_equal(v.view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(n.view(np.uint32), pm.quat_rotate(T[:4], m[3]).view(np.uint32))
    ln = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.all(np.abs(ln[ln > 0] - 1) < 1e-5)


def test_rainbow_color_map_hand_worked():
    assert sr.rainbow_color_map(0).tolist() == [255, 0, 0, 255]
    assert sr.rainbow_color_map(1 / 6).tolist() == [255, 255, 0, 255]    # (1/6) * 6 rounds to 1.0 exactly
    assert sr.rainbow_color_map(0.5).tolist() == [0, 255, 255, 255]
    assert sr.rainbow_color_map(1).tolist() == [255, 0, 0, 255]          # h - floor(h)
    assert sr.rainbow_color_map(1 / 12).tolist() == [255, 127, 0, 255]   # 255 * 0.5 truncated
    assert sr.submap_color(10).tolist() == [0, 255, 255, 255]            # 10 / 20 = 0.5
    assert sr.submap_color(20).tolist() == sr.submap_color(0).tolist()   # the cycle


def test_capi_rainbow_color_map_equals_the_restatement():
    rng = np.random.default_rng(0)
    hs = np.concatenate([rng.uniform(-3, 3, 2000), np.arange(-40, 80) / 20.0, np.arange(0, 25) / 24.0])
    for h in hs:
        assert np.array_equal(capi.rainbow_color_map(h), sr.rainbow_color_map(h)), h
    for i in range(-5, 60):
        assert np.array_equal(capi.submap_color(i), sr.submap_color(i)), i
    assert capi.DEFAULT_COLOR_CYCLE_LENGTH == 20


def test_symbols_exported_and_null_context_refused_without_a_device():
    lib = capi.load()
    for name in ("vgx_submaps_generate_separated_mesh", "vgx_mesh_has_colors", "vgx_mesh_download_colors"):
        assert hasattr(lib, name), name
    T = np.array([1, 0, 0, 0, 0, 0, 0], F)
    rgba = np.zeros(4, np.uint8)
    arr = (C.c_void_p * 1)(None)
    rc = lib.vgx_submaps_generate_separated_mesh(None, 0, arr, T.ctypes.data_as(C.POINTER(C.c_float)),
                                                 rgba.ctypes.data_as(C.POINTER(C.c_uint8)), None, None)
    assert rc == capi.ERR_INVALID
    has = C.c_int32(7)
    assert lib.vgx_mesh_has_colors(None, C.byref(has)) == capi.ERR_INVALID and has.value == 7
    assert lib.vgx_mesh_download_colors(None, rgba.ctypes.data_as(C.POINTER(C.c_uint8))) == capi.ERR_INVALID
