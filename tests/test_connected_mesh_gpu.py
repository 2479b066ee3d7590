"""vgx_mesh_connect (voxblox createConnectedMesh) on the device: bit for bit against the numpy restatement of
tests/connected_mesh_ref.py through the C ABI -- a layer mesh and a submap mesh at three thresholds, a separated mesh
with colours, another upload order, run to run, a reused handle going large, small, large, the untouched source, the
empty mesh, every refusal (the out-of-range flag among them) and the PLY file.
Not provoked here: the refusal of a source handle whose last generating call failed after it had reset the handle (an
allocation or device failure); the flag behind it is set on the paths the other refusals do not reach."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import connected_mesh_ref as cr
from tests.test_mesh_cpu import edge_case_layer, sphere_layer
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _want(mesh, thr):
    _, _, v, n = mesh.download()
    colors = mesh.download_colors() if mesh.has_colors() else None
    return cr.connect(v, n, colors, thr)


def _assert_equal(got, want):
    for name, g, w in zip(("vertices", "normals", "rgba", "indices"), got, want):
        assert (g is None) == (w is None), name
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())
        assert len(bad) == 0, (name, len(bad), bad[:5])


def _check(mesh, thr, out, min_tris=1000):
    mesh.connect(thr, out)
    want = _want(mesh, thr)
    nv, nt, has = out.stats()
    assert (nv, nt, has) == (len(want[0]), len(want[3]), mesh.has_colors()) and nt >= min_tris
    assert nv <= 0.5 * 3 * nt, nv / (3 * nt)                    # something was welded
    _assert_equal(out.download(), want)
    return want


def _thresholds(vs):
    return (F(1e-10), F(0.5) * F(vs), F(0.013))


@pytest.mark.parametrize("vps,seed", [(8, 0), (16, 1)])
def test_layer_and_submap_meshes_bit_exact(ctx, vps, seed):
    rng = np.random.default_rng(seed)
    vs = 0.2 if vps == 8 else 0.1
    data = edge_case_layer(rng, vps, (-2, -2, -1), (4, 3, 3) if vps == 8 else (2, 2, 2), density=0.7)
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.upload(*data)
    sm = capi.Submap(ctx, 1, vs, vps, *data)
    out = capi.ConnectedMesh(ctx)
    for mesh in (layer.generate_mesh(), sm.generate_mesh()):
        for thr in _thresholds(vs):
            _check(mesh, thr, out)
        mesh.destroy()
    # analytic spheres, at the origin and far from it (cells of 1e-10 there: 4e11 and beyond)
    for centre in ((0.0, 0.0, 0.0), (40.0, -30.0, 10.0)):
        sp = capi.Submap(ctx, 2, 0.1, vps, *sphere_layer(centre, 0.95, vps, 0.1))
        mesh = sp.generate_mesh()
        for thr in _thresholds(0.1):
            _check(mesh, thr, out)
        mesh.destroy()
        sp.destroy()
    out.destroy()
    sm.destroy()
    layer.destroy()


def _yaw(yaw, t):
    return np.array([math.cos(yaw / 2), 0, 0, math.sin(yaw / 2), *t], F)


def _separated(ctx, rng, n_sub=4):
    subs = [edge_case_layer(rng, 8, (-2 + k % 2, -1 - k % 2, -1), (3, 3, 2), density=0.8) for k in range(n_sub)]
    handles = [capi.Submap(ctx, k, 0.2, 8, *s) for k, s in enumerate(subs)]
    T = np.stack([_yaw(0.2 * k - 0.3, (0.4 * k, -0.2 * k, 0.1)) for k in range(n_sub)])
    rgba = rng.integers(0, 256, (n_sub, 4), dtype=np.uint8)
    return subs, handles, T, rgba


def test_separated_mesh_with_colours_bit_exact(ctx):
    rng = np.random.default_rng(4)
    subs, handles, T, rgba = _separated(ctx, rng)
    mesh = capi.Mesh(ctx).generate_separated(handles, T, rgba)
    bi, first, _, _ = mesh.download()
    colors = mesh.download_colors()
    # shared block indices: an output block holds triangles of several submaps, so first occurrence crosses submaps
    mixed = sum(len(np.unique(colors[first[k]:first[k + 1]], axis=0)) > 1 for k in range(len(bi)))
    assert mixed > 3
    out = capi.ConnectedMesh(ctx)
    for thr in _thresholds(0.2):
        want = _check(mesh, thr, out)
        assert want[2] is not None and len(np.unique(want[2], axis=0)) == len(subs)
    # identity poses: the submaps' copies of a shared block weld across submaps, and the first submap's colour wins
    I = np.tile(_yaw(0.0, (0, 0, 0)), (2, 1))
    mesh.generate_separated([handles[0], handles[0]], I, rgba[:2])
    want = _check(mesh, F(1e-10), out)
    assert (want[2] == rgba[0]).all() and len(want[0]) <= 0.25 * 3 * len(want[3])
    out.destroy()
    mesh.destroy()
    for h in handles:
        h.destroy()


def test_upload_order_runs_and_reuse(ctx):
    rng = np.random.default_rng(9)
    vs, vps = 0.2, 8
    bi, d, w = edge_case_layer(rng, vps, (-1, -2, 0), (4, 3, 2), density=0.8)
    small = edge_case_layer(rng, vps, (0, 0, 0), (2, 2, 2), density=1.0)
    thr = F(0.05)
    outs = []
    for perm in (np.arange(len(bi)), rng.permutation(len(bi))):
        layer = capi.TsdfLayer(ctx, vs, vps)
        layer.upload(bi[perm], d[perm], w[perm])
        mesh = layer.generate_mesh()
        outs.append(mesh.connect(thr).download())
        mesh.destroy()
        layer.destroy()
    _assert_equal(outs[1], outs[0])                                  # the same layer in another block order
    big_sm, small_sm = capi.Submap(ctx, 1, vs, vps, bi, d, w), capi.Submap(ctx, 2, vs, vps, *small)
    big, sml = big_sm.generate_mesh(), small_sm.generate_mesh()
    src_before = big.download()
    out = capi.ConnectedMesh(ctx)
    a = _check(big, thr, out)
    _assert_equal(a, outs[0])                                        # the submap's mesh is the layer's
    big.connect(thr, out)
    _assert_equal(out.download(), a)                                 # two runs, the same bytes
    fresh_small = sml.connect(thr).download()
    _check(sml, thr, out, min_tris=100)                              # large, small ...
    _assert_equal(out.download(), fresh_small)
    assert len(fresh_small[3]) < len(a[3])
    _check(big, thr, out)                                            # ... large
    _assert_equal(out.download(), a)
    _check(big, F(1e-10), out)
    for g, s in zip(big.download(), src_before):                     # the source is not changed
        assert np.array_equal(g.view(np.uint8), s.view(np.uint8))
    assert not big.has_colors()
    # an empty mesh: no blocks, and blocks without a surface
    empty = capi.Mesh(ctx)
    big.connect(thr, out)
    empty.connect(thr, out)
    assert out.stats() == (0, 0, False)
    assert [x.shape for x in out.download() if x is not None] == [(0, 3), (0, 3), (0, 3)]
    flat = capi.Submap(ctx, 3, vs, vps, bi[:3], np.full((3, vps ** 3), 0.25, F), np.ones((3, vps ** 3), F))
    flat.generate_mesh(empty)
    assert empty.stats() == (3, 0)
    big.connect(thr, out)
    empty.connect(thr, out)
    assert out.stats() == (0, 0, False)
    empty.generate_separated([flat], _yaw(0.1, (0, 0, 0))[None], np.array([[1, 2, 3, 4]], np.uint8))
    empty.connect(thr, out)
    assert out.stats() == (0, 0, True) and out.download()[2].shape == (0, 4)
    for o in (out, empty, big, sml, big_sm, small_sm, flat):
        o.destroy()


def test_refusals(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(11)
    data = edge_case_layer(rng, 8, (0, 0, 0), (2, 2, 2), density=1.0)
    sm = capi.Submap(ctx, 1, 0.2, 8, *data)
    mesh = sm.generate_mesh()
    out = capi.ConnectedMesh(ctx)
    thr = F(0.01)
    before = _check(mesh, thr, out, min_tris=100)

    def refused(code, m, t, o, say=None, keeps=True):
        assert lib.vgx_mesh_connect(m, C.c_float(t), o) == code
        if say is not None:
            assert say in lib.vgx_last_error(ctx.h).decode()
        if keeps:                                                    # refused before anything is launched
            _assert_equal(out.download(), before)

    I = capi.ERR_INVALID
    refused(I, None, thr, out.h)
    refused(I, mesh.h, thr, None, say="NULL connected mesh")
    other = capi.Context(0)
    out2 = capi.ConnectedMesh(other)
    refused(I, mesh.h, thr, out2.h, say="another context")
    for bad in (0.0, -0.0, -1e-10, float("nan"), float("inf"), -float("inf")):
        refused(I, mesh.h, bad, out.h, say="threshold")
    with pytest.raises(capi.VgxError) as e:
        n = np.zeros((out.stats()[0], 4), np.uint8)
        ctx.check(lib.vgx_connected_mesh_download(out.h, None, None, n.ctypes.data_as(C.POINTER(C.c_uint8)), None))
    assert e.value.code == I                                         # rgba asked of a mesh without colours
    # the out-of-range flag: ordinary coordinates, a threshold so small that |v * inv| >= 2^62
    refused(capi.ERR_UNSUPPORTED, mesh.h, 1e-30, out.h, say="2^62", keeps=False)
    assert out.stats() == (0, 0, False)                              # the handle holds no mesh
    _check(mesh, thr, out, min_tris=100)                             # and the next valid call works
    _assert_equal(out.download(), before)
    # just inside the range: |v| <= 3.2 m here, and 2^62 cells of 2e-18 m reach 9.2 m
    _check(mesh, F(2e-18), out, min_tris=100)
    refused(capi.ERR_UNSUPPORTED, mesh.h, 1e-19, out.h, say="2^62", keeps=False)
    assert out.stats() == (0, 0, False)
    assert lib.vgx_connected_mesh_write_ply(out.h, None) == I
    assert lib.vgx_connected_mesh_write_ply(out.h, b"/nonexistent-directory/x.ply") == I
    for o in (out2, out, mesh, sm):
        o.destroy()
    other.close()


def _parse_ply(raw, colored):
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode().split("\n")
    vdt = np.dtype([("p", "<f4", 3), ("n", "<f4", 3)] + ([("c", "u1", 4)] if colored else []))
    V = int([h for h in header if h.startswith("element vertex ")][0].split()[-1])
    T = int([h for h in header if h.startswith("element face ")][0].split()[-1])
    vert = np.frombuffer(raw[end:end + V * vdt.itemsize], vdt)
    faces = np.frombuffer(raw[end + V * vdt.itemsize:], np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert len(faces) == T
    return header, vert, faces


def test_ply_equals_the_download(ctx, tmp_path):
    rng = np.random.default_rng(3)
    _, handles, T, rgba = _separated(ctx, rng, 3)
    mesh = capi.Mesh(ctx).generate_separated(handles, T, rgba)
    out = mesh.connect(F(0.1))
    base = ["property float x", "property float y", "property float z", "property float nx", "property float ny",
            "property float nz"]
    col = ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    for colored in (True, False):
        if not colored:
            handles[0].generate_mesh(mesh)
            mesh.connect(F(0.1), out)
        v, n, c, idx = out.download()
        path = tmp_path / f"connected{int(colored)}.ply"
        out.write_ply(str(path))
        header, vert, faces = _parse_ply(path.read_bytes(), colored)
        assert header[:2] == ["ply", "format binary_little_endian 1.0"]
        assert [h for h in header if h.startswith("property")] == base + (col if colored else []) + [
            "property list uchar int vertex_indices"]
        assert f"element vertex {len(v)}" in header and f"element face {len(idx)}" in header and len(v) > 100
        assert np.array_equal(vert["p"].view(np.uint32), v.view(np.uint32))
        assert np.array_equal(vert["n"].view(np.uint32), n.view(np.uint32))
        assert (c is not None) == colored and (not colored or np.array_equal(vert["c"], c))
        assert (faces["n"] == 3).all() and np.array_equal(faces["i"].astype(np.uint32), idx)
        # the soup's file is larger, and vgx_mesh_write_ply is what it was: faces (3t, 3t+1, 3t+2)
        soup = tmp_path / f"soup{int(colored)}.ply"
        mesh.write_ply(str(soup))
        assert soup.stat().st_size > path.stat().st_size
        assert f"element vertex {3 * len(idx)}".encode() in soup.read_bytes()[:200]
    out.destroy()
    mesh.destroy()
    for h in handles:
        h.destroy()
