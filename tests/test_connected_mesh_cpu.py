"""The connected mesh without a device: the numpy restatement (tests/connected_mesh_ref.py) checked by properties that do
not trust it, on meshes tests/mesh_ref.py makes of an analytic sphere (at the origin and far from it) and of a random
layer with the planted corner cases; against a literal dict-and-loop transcription of voxblox's createConnectedMesh
[recalled] that rounds with libm's round; a hand-worked case for the rounding; and the C ABI's new symbols."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from tests import connected_mesh_ref as cr
from tests import mesh_ref as mr
from tests.test_mesh_cpu import edge_case_layer, sphere_layer
from voxgraph_amd import capi

F = np.float32


def _scene(name):
    if name == "sphere":
        vs, layer = 0.1, sphere_layer((0.0, 0.0, 0.0), 0.95, 8, 0.1)
    elif name == "sphere_far":
        vs, layer = 0.1, sphere_layer((40.0, -30.0, 10.0), 0.95, 8, 0.1)
    else:
        vs, layer = 0.2, edge_case_layer(np.random.default_rng(0), 8, (-2, -2, -1), (4, 3, 3), density=0.7)
    _, _, v, n, _ = mr.generate_mesh(*layer, 8, vs)
    return vs, v, n


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = _scene(name)
    return _CACHE[name]


SCENES = ("sphere", "sphere_far", "edge_cases")


def _thresholds(vs):
    return (F(1e-10), F(0.5) * F(vs))


@pytest.mark.parametrize("name", SCENES)
def test_properties_of_the_restatement(name):
    vs, v, n = _case(name)
    soup = v.reshape(-1, 3)
    colors = (np.arange(len(v))[:, None] * np.array([1, 3, 5, 7]) % 256).astype(np.uint8)
    for thr in _thresholds(vs):
        uv, un, uc, idx = cr.connect(v, n, colors, thr)
        assert idx.shape == (len(v), 3) and idx.dtype == np.uint32 and uv.dtype == F
        # the tests weld something: they cannot pass on an identity mapping
        assert len(uv) <= 0.5 * len(soup), (name, thr, len(uv) / len(soup))
        k_soup = cr.keys(soup, thr)
        k_out = cr.keys(uv, thr)
        # every output key is distinct
        assert len({tuple(k) for k in k_out.tolist()}) == len(uv)
        # each unique vertex is bitwise soup vertex min{j : key(j) = its key}, and they come in ascending j
        first = {}
        for j, k in enumerate(map(tuple, k_soup.tolist())):
            first.setdefault(k, j)
        js = np.array([first[tuple(k)] for k in k_out.tolist()])
        assert np.all(np.diff(js) > 0) and len(first) == len(uv)
        assert np.array_equal(uv.view(np.uint32), soup[js].view(np.uint32))
        assert np.array_equal(un.view(np.uint32), n[js // 3].view(np.uint32))
        assert np.array_equal(uc, colors[js // 3])
        # vertices[indices] lies in the cell of the soup vertex it replaces: within the threshold per axis
        flat = idx.reshape(-1)
        assert flat.max() == len(uv) - 1
        assert np.array_equal(k_out[flat], k_soup)
        assert np.all(np.abs(uv[flat].astype(np.float64) - soup.astype(np.float64)) <= np.float64(thr))
    # at 1e-10f an f32 step above 0.01 is far above the cell: such vertices only weld with bitwise copies
    uv, _, _, idx = cr.connect(v, n, None, F(1e-10))
    big = np.all(np.abs(soup) > 0.01, axis=1)
    assert big.sum() > 100
    assert np.array_equal(uv[idx.reshape(-1)][big].view(np.uint32), soup[big].view(np.uint32))


def _libm_round():
    lib = C.CDLL(ctypes.util.find_library("m"))
    lib.round.restype = C.c_double
    lib.round.argtypes = [C.c_double]
    return lib.round


def literal_connected_mesh(v, n, colors, threshold):
    """createConnectedMesh [recalled], one vertex at a time: a map from the LongIndex of the vertex to its new index"""
    rnd = _libm_round()
    inv = 1.0 / float(F(threshold))
    uniques = {}
    verts, norms, cols, indices = [], [], [], []
    for t in range(len(v)):
        for c in range(3):
            p = v[t, c]
            key = tuple(int(rnd(float(p[a]) * inv)) for a in range(3))
            at = uniques.get(key)
            if at is None:
                at = len(verts)
                uniques[key] = at
                verts.append(p)
                norms.append(n[t])
                cols.append(colors[t])
            indices.append(at)
    return (np.array(verts, F).reshape(-1, 3), np.array(norms, F).reshape(-1, 3), np.array(cols, np.uint8).reshape(-1, 4),
            np.array(indices, np.uint32).reshape(-1, 3))


@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_literal_transcription(name):
    vs, v, n = _case(name)
    colors = (np.arange(len(v))[:, None] * np.array([7, 5, 3, 1]) % 256).astype(np.uint8)
    for thr in _thresholds(vs) + (F(0.013),):
        got = cr.connect(v, n, colors, thr)
        want = literal_connected_mesh(v, n, colors, thr)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8))


def test_rounding_hand_worked():
    # threshold 0.5f: inv = 2.0 exactly, so x * inv is exactly +-0.5, +-1.5, -0.0
    x = np.array([0.25, -0.25, 0.75, -0.75, -0.0, 0.0, 1.25, -1.25], F)
    pts = np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)
    assert cr.keys(pts, F(0.5))[:, 0].tolist() == [1, -1, 2, -2, 0, 0, 3, -3]       # np.round: 0, -0, 2, -2, ., ., 2, -2
    assert np.round(np.float64(0.5)) == 0 and cr.round_half_away(np.float64(0.5)) == 1
    assert cr.round_half_away(np.float64(0.49999999999999994)) == 0                   # (floor(x + 0.5) says 1)
    # -0.0 and +0.0 weld; the first copy's bits are kept
    v = np.array([[[-0.0, 0.0, 0.0], [1, 0, 0], [0, 1, 0]], [[0.0, -0.0, 0.0], [0, 1, 0], [1, 0, 0]]], F)
    n = np.array([[0, 0, 1], [0, 0, -1]], F)
    uv, un, uc, idx = cr.connect(v, n, None, F(1e-10))
    assert uc is None and idx.tolist() == [[0, 1, 2], [0, 2, 1]]
    assert np.array_equal(uv.view(np.uint32), v[0].view(np.uint32)) and np.signbit(uv[0, 0])
    assert np.array_equal(un, n[[0, 0, 0]])
    # a triangle whose corners weld together is kept
    v = np.array([[[0.1, 0.1, 0.1], [0.12, 0.1, 0.1], [0.1, 0.12, 0.1]]], F)
    uv, _, _, idx = cr.connect(v, n[:1], None, F(0.5))
    assert len(uv) == 1 and idx.tolist() == [[0, 0, 0]]
    # refusals of the restatement are the library's
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            cr.keys(pts, bad)
    with pytest.raises(OverflowError):
        cr.keys(pts + F(1), F(1e-30))
    with pytest.raises(OverflowError):
        cr.keys(np.array([[np.nan, 0, 0]], F), F(0.1))
    empty = cr.connect(np.zeros((0, 3, 3), F), np.zeros((0, 3), F), np.zeros((0, 4), np.uint8), F(0.1))
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0, 4), (0, 3)]


def test_symbols_exported_and_null_handles_refused_without_a_device():
    lib = capi.load()
    names = ("vgx_connected_mesh_create", "vgx_connected_mesh_destroy", "vgx_mesh_connect", "vgx_connected_mesh_stats",
             "vgx_connected_mesh_download", "vgx_connected_mesh_write_ply")
    for name in names:
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert hasattr(capi, "ConnectedMesh") and hasattr(capi.Mesh, "connect")
    out = C.c_void_p(5)
    assert lib.vgx_connected_mesh_create(None, C.byref(out)) == capi.ERR_INVALID and out.value == 5
    assert lib.vgx_connected_mesh_destroy(None) == capi.ERR_INVALID
    assert lib.vgx_mesh_connect(None, C.c_float(1e-10), None) == capi.ERR_INVALID
    nv = C.c_int64(7)
    assert lib.vgx_connected_mesh_stats(None, C.byref(nv), None, None) == capi.ERR_INVALID and nv.value == 7
    assert lib.vgx_connected_mesh_download(None, None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_connected_mesh_write_ply(None, b"/nonexistent/x.ply") == capi.ERR_INVALID
