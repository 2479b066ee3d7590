"""vgx_tsdf_layer_generate_mesh / vgx_submap_generate_mesh (the combined mesh, voxblox MeshIntegrator::generateMesh) on
the device: bit for bit against the numpy restatement of tests/mesh_ref.py, and against properties that do not trust it
-- closed spheres, the isosurface points of the same data, run-to-run identity, the PLY file."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_ref as mr
from tests.test_mesh_cpu import check_sphere, edge_case_layer, sphere_layer
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _layer(ctx, vs, vps, bi, d, w):
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.upload(bi, d, w)
    return layer


def _assert_mesh_equal(got, want):
    names = ("block_index", "first", "vertices", "normals")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())
        assert len(bad) == 0, (name, len(bad), bad[:5])


def _edge_keys(v, vs):
    """grid edge of every vertex from the positions alone: the triangle's centroid lies in the cube that made it, and each
    vertex on the nearest of that cube's 12 edges (an edge on a cube face is shared with the neighbour cube: a centroid on
    a face picks either, with the same keys)"""
    p = v.astype(np.float64) / vs - 0.5                                # voxel-centre units
    cube = np.floor(p.mean(1)).astype(np.int64)                         # [T][3]
    A = cube[:, None, :] + mr.CORNERS[mr.EDGES[:, 0]]                   # [T][12][3]
    B = cube[:, None, :] + mr.CORNERS[mr.EDGES[:, 1]]
    lo, hi = np.minimum(A, B), np.maximum(A, B)
    keys = np.zeros(v.shape[:2] + (4,), np.int64)
    for q in range(3):
        x = p[:, q, None, :]
        gap = np.maximum(lo - x, 0) + np.maximum(x - hi, 0)
        e = np.argmin((gap ** 2).sum(-1), 1)                           # [T]
        assert ((gap[np.arange(len(e)), e] ** 2).sum(-1) < 1e-8).all()  # on that edge, to f32 rounding
        keys[:, q, :3] = lo[np.arange(len(e)), e]
        keys[:, q, 3] = np.argmax(hi[np.arange(len(e)), e] != lo[np.arange(len(e)), e], 1)
    return keys


@pytest.mark.parametrize("vps,seed", [(8, 0), (8, 1), (16, 2)])
def test_random_layer_bit_exact(ctx, vps, seed):
    rng = np.random.default_rng(seed)
    vs = 0.1 if vps == 16 else 0.2
    bi, d, w = edge_case_layer(rng, vps, (-2, -2, -1), (4, 3, 3) if vps == 8 else (3, 2, 2), density=0.7)
    layer = _layer(ctx, vs, vps, bi, d, w)
    mesh = layer.generate_mesh()
    got = mesh.download()
    want = mr.generate_mesh(bi, d, w, vps, vs, 1e-4)[:4]
    assert mesh.stats() == (len(bi), len(want[2])) and len(want[2]) > 1000
    _assert_mesh_equal(got, want)
    # other thresholds
    for mw in (0.0, 2.0):
        layer.generate_mesh(mesh, min_weight=mw)
        _assert_mesh_equal(mesh.download(), mr.generate_mesh(bi, d, w, vps, vs, mw)[:4])
    # the same blocks uploaded in another order: the same mesh
    perm = rng.permutation(len(bi))
    shuffled = _layer(ctx, vs, vps, bi[perm], d[perm], w[perm])
    _assert_mesh_equal(shuffled.generate_mesh().download(), want)
    # the submap source on the same data
    sm = capi.Submap(ctx, 3, vs, vps, bi, d, w)
    _assert_mesh_equal(sm.generate_mesh().download(), want)
    sm.destroy()
    mesh.destroy()
    layer.destroy()
    shuffled.destroy()


def _box_scan():
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, 256, endpoint=False) + (2 * np.pi / 256) / 3.0,
                         np.linspace(-0.3, 0.3, 12) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    lo, hi = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    return (d * t[:, None]).astype(F)


def test_reproducible_scan_layer(ctx):
    layer = capi.TsdfLayer(ctx, 0.2, 16)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for k in range(3):
        T = np.array([1, 0, 0, 0, 0.1 + 0.2 * k, -0.05, 0.02], F)
        integ.integratePointCloud(T, _box_scan(), count=False)
    mesh = layer.generate_mesh()       # (queued behind the scans on the TSDF stream: no explicit wait)
    bi, d, w, _ = layer.download()
    want = mr.generate_mesh(bi, d, w, 16, 0.2, 1e-4)[:4]
    assert len(want[2]) > 1000
    _assert_mesh_equal(mesh.download(), want)
    integ.destroy()
    mesh.destroy()
    layer.destroy()


def _yaw_pose(yaw, t):
    return np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)


def test_city_projected_map(ctx):
    """24 city submaps at 128^3 voxels: the combined mesh of their projected map against the restatement"""
    vs, vps = 0.1, 16
    handles, T = [], []
    for k in range(24):
        p = np.array([1.6 * k, 0.4 * np.sin(k), 0.05 * k, 0.15 * k])
        handles.append(capi.Submap.synth_city(ctx, k, vs, vps, (-4, -4, -4), (8, 8, 8), 0.3, 2.0, 10.0, p, 3))
        T.append(_yaw_pose(p[3], p[:3]))
    T = np.stack(T)
    layer = capi.TsdfLayer(ctx, vs, vps)
    mesh = capi.combined_mesh(ctx, handles[::-1], T[::-1], layer)
    bi, d, w, _ = layer.download()
    want = mr.generate_mesh(bi, d, w, vps, vs, 1e-4)[:4]
    assert len(want[0]) > 500 and len(want[2]) > 10000
    _assert_mesh_equal(mesh.download(), want)
    # one submap's own mesh, in the submap frame
    td, tw, _, _ = handles[5].download_layers(vps)
    _assert_mesh_equal(handles[5].generate_mesh(mesh).download(),
                       mr.generate_mesh(handles[5].block_index(), td, tw, vps, vs, 1e-4)[:4])
    for h in handles:
        h.destroy()
    mesh.destroy()
    layer.destroy()


@pytest.mark.parametrize("radius_vox,seed", [(6.5, 3), (11, 4), (17, 5)])
def test_sphere_on_device(ctx, radius_vox, seed):
    rng = np.random.default_rng(seed)
    vps = 8 if seed % 2 else 16
    vs = 0.1
    centre = rng.uniform(-0.5, 0.5, 3)
    bi, d, w = sphere_layer(centre, radius_vox * vs, vps, vs)
    layer = _layer(ctx, vs, vps, bi, d, w)
    mesh = layer.generate_mesh()
    gbi, first, v, n = mesh.download()
    check_sphere((gbi, first, v, n, _edge_keys(v, vs)), centre, radius_vox * vs)
    mesh.destroy()
    layer.destroy()


def test_isosurface_points_lie_on_mesh_vertices(ctx):
    rng = np.random.default_rng(8)
    vps, vs, mw = 16, 0.1, 0.5
    centre = rng.uniform(-0.3, 0.3, 3)
    bi, d, w = sphere_layer(centre, 1.3, vps, vs)
    d = np.clip(d, -0.3, 0.3).astype(F)
    w = rng.uniform(0.1, 3.0, w.shape).astype(F)                    # some cubes fall below min_weight
    sm = capi.Submap(ctx, 1, vs, vps, bi, d, w)
    n_iso = sm.extract_isosurface_points(min_voxel_weight=mw)
    iso = sm.download_points(capi.POINTS_ISOSURFACE)[0].reshape(-1, 3)
    _, _, v, _ = sm.generate_mesh(min_weight=mw).download()
    assert n_iso > 100 and len(v) > 100
    # every isosurface point within 1e-5 voxel of a mesh vertex (cells of that size: the point's cell and its neighbours)
    tol = 1e-5 * vs
    cells = {}
    for p in v.reshape(-1, 3).astype(np.float64):
        cells.setdefault(tuple(np.floor(p / tol).astype(np.int64)), []).append(p)
    offsets = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for p in iso.astype(np.float64):
        c = np.floor(p / tol).astype(np.int64)
        near = [q for o in offsets for q in cells.get(tuple(c + o), [])]
        assert near and np.abs(np.array(near) - p).max(1).min() <= tol, p
    sm.destroy()


def test_run_to_run_and_reuse(ctx):
    rng = np.random.default_rng(12)
    big = edge_case_layer(rng, 16, (-2, -2, -2), (4, 4, 3), density=0.9)
    small = edge_case_layer(rng, 16, (0, 0, 0), (2, 2, 1), density=1.0)
    lb, ls = _layer(ctx, 0.1, 16, *big), _layer(ctx, 0.1, 16, *small)
    m = capi.Mesh(ctx)
    lb.generate_mesh(m)
    a = m.download()
    lb.generate_mesh(m)
    _assert_mesh_equal(m.download(), a)
    ls.generate_mesh(m)                                               # a smaller mesh into the grown handle
    fresh = ls.generate_mesh()
    _assert_mesh_equal(m.download(), fresh.download())
    assert m.stats() == fresh.stats() and m.stats()[1] < len(a[2])
    for h in (m, fresh, lb, ls):
        h.destroy()


def test_errors_and_edge_cases(ctx):
    lib = ctx.lib
    layer = capi.TsdfLayer(ctx, 0.1, 8)
    m = capi.Mesh(ctx)
    assert m.stats() == (0, 0)
    # an empty layer: OK, 0 blocks
    layer.generate_mesh(m)
    assert m.stats() == (0, 0)
    bi, first, v, n = m.download()
    assert bi.shape == (0, 3) and list(first) == [0] and v.shape == (0, 3, 3)
    rng = np.random.default_rng(1)
    data = edge_case_layer(rng, 8, (0, 0, 0), (2, 2, 2), density=1.0)
    layer.upload(*data)
    layer.generate_mesh(m)
    before = m.download()
    assert len(before[2]) > 0
    cfg = capi.MeshConfig(1e-4)
    assert lib.vgx_tsdf_layer_generate_mesh(None, C.byref(cfg), m.h) == capi.ERR_INVALID
    assert lib.vgx_tsdf_layer_generate_mesh(layer.h, C.byref(cfg), None) == capi.ERR_INVALID
    assert lib.vgx_submap_generate_mesh(None, C.byref(cfg), m.h) == capi.ERR_INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        rc = lib.vgx_tsdf_layer_generate_mesh(layer.h, C.byref(capi.MeshConfig(bad)), m.h)
        assert rc == capi.ERR_INVALID and "min_weight" in lib.vgx_last_error(ctx.h).decode()
    other = capi.Context(0)
    m2 = capi.Mesh(other)
    assert lib.vgx_tsdf_layer_generate_mesh(layer.h, C.byref(cfg), m2.h) == capi.ERR_INVALID
    _assert_mesh_equal(m.download(), before)                          # refusals wrote nothing
    assert lib.vgx_tsdf_layer_generate_mesh(layer.h, None, m.h) == capi.OK   # NULL config: the defaults
    _assert_mesh_equal(m.download(), before)
    # released raw layers
    sm = capi.Submap(ctx, 4, 0.1, 8, *data)
    sm.generate_mesh(m)
    _assert_mesh_equal(m.download(), before)
    sm.release_raw_layers()
    with pytest.raises(capi.VgxError) as e:
        sm.generate_mesh(m)
    assert e.value.code == capi.ERR_INVALID
    _assert_mesh_equal(m.download(), before)
    sm.destroy()
    m2.destroy()
    other.close()
    m.destroy()
    layer.destroy()


def test_ply_roundtrip(ctx, tmp_path):
    rng = np.random.default_rng(3)
    data = edge_case_layer(rng, 8, (-1, -1, 0), (3, 2, 2), density=1.0)
    layer = _layer(ctx, 0.2, 8, *data)
    m = layer.generate_mesh()
    _, _, v, n = m.download()
    path = tmp_path / "mesh.ply"
    m.write_ply(str(path))
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode().split("\n")
    T = len(v)
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {3 * T}" in header and f"element face {T}" in header
    assert "property list uchar int vertex_indices" in header
    vert = np.frombuffer(raw[end:end + 3 * T * 24], "<f4").reshape(T, 3, 6)
    assert np.array_equal(vert[..., :3].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(vert[..., 3:].view(np.uint32), np.repeat(n[:, None, :], 3, 1).view(np.uint32))
    faces = np.frombuffer(raw[end + 3 * T * 24:], np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert len(faces) == T and (faces["n"] == 3).all()
    assert np.array_equal(faces["i"].ravel(), np.arange(3 * T))
    m.destroy()
    layer.destroy()
