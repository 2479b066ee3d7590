"""vgx_submaps_generate_separated_mesh (cblox generateSeparatedMesh) on the device: bit for bit against the numpy
restatement of tests/separated_mesh_ref.py, against vgx_submap_generate_mesh at the identity, run to run, through a
reused handle, after and before the single-layer calls, on every refusal, in the PLY file, and on a city-scale sample."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import mesh_ref as mr
from tests import separated_mesh_ref as sr
from tests.test_mesh_cpu import edge_case_layer
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _download(mesh):
    return mesh.download() + (mesh.download_colors(),)


def _assert_equal(got, want):
    names = ("block_index", "first", "vertices", "normals", "colors")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())
        assert len(bad) == 0, (name, len(bad), bad[:5])


def _yaw(yaw, t):
    return np.array([math.cos(yaw / 2), 0, 0, math.sin(yaw / 2), *t], F)


def _general(rng, t):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.array([*q, *t], F)


def _random_subs(rng, vps):
    """five random layers over overlapping block boxes, and one whose blocks hold no surface"""
    subs = []
    for k in range(5):
        lo = (-2 + k % 2, -1 - k % 3, -1)
        subs.append(edge_case_layer(rng, vps, lo, (3, 3, 2) if vps == 8 else (2, 2, 2), density=0.7))
    bi = np.array([(0, 0, 0), (1, 0, 0), (5, 5, 5)], np.int32)
    d = np.full((3, vps ** 3), 0.25, F)
    subs.append((bi, d, np.ones_like(d)))
    return subs


@pytest.mark.parametrize("vps,seed", [(8, 0), (16, 1)])
def test_random_submaps_bit_exact(ctx, vps, seed):
    rng = np.random.default_rng(seed)
    vs = 0.2 if vps == 8 else 0.1
    subs = _random_subs(rng, vps)
    handles = [capi.Submap(ctx, 10 + k, vs, vps, *s) for k, s in enumerate(subs)]
    poses = [_yaw(0.3 * k - 0.7, (0.5 * k, -0.25 * k, 0.1)) for k in range(3)]
    poses += [_general(rng, (0.2 * k, 0.4, -0.3)) for k in range(3)]
    colors = rng.integers(0, 256, (len(subs), 4), dtype=np.uint8)
    mesh = capi.Mesh(ctx)
    orders = [list(range(len(subs))), [3, 1, 1, 5, 0, 2, 4], list(rng.permutation(len(subs)))]
    for order in orders:                                  # array order, a duplicate, a shuffle
        T = np.stack([poses[i] for i in order])
        rgba = colors[order]
        mesh.generate_separated([handles[i] for i in order], T, rgba)
        assert mesh.has_colors()
        want = sr.separated_mesh([subs[i] for i in order], T, rgba, vps, vs)
        assert len(want[2]) > 1000 and mesh.stats() == (len(want[0]), len(want[2]))
        _assert_equal(_download(mesh), want)
    # another threshold
    mesh.generate_separated(handles, np.stack(poses), colors, min_weight=2.0)
    _assert_equal(_download(mesh), sr.separated_mesh(subs, np.stack(poses), colors, vps, vs, 2.0))
    # the module-level call: ascending IDs, voxgraph's colours by default
    rev = handles[::-1]
    capi.separated_mesh(ctx, rev, np.stack(poses[::-1]), mesh=mesh)
    want = sr.separated_mesh(subs, np.stack(poses), np.stack([sr.submap_color(10 + k) for k in range(len(subs))]), vps, vs)
    _assert_equal(_download(mesh), want)
    mesh.destroy()
    for h in handles:
        h.destroy()


def test_one_submap_at_identity_equals_the_submap_mesh(ctx):
    rng = np.random.default_rng(5)
    data = edge_case_layer(rng, 16, (-1, -2, 0), (3, 2, 2), density=0.8)
    sm = capi.Submap(ctx, 3, 0.1, 16, *data)
    single = sm.generate_mesh().download()
    mesh = capi.Mesh(ctx).generate_separated([sm], np.array([[1, 0, 0, 0, 0, 0, 0]], F), np.array([[9, 8, 7, 6]], np.uint8))
    bi, first, v, n, rgba = _download(mesh)
    assert len(v) > 1000
    assert np.array_equal(bi, single[0]) and np.array_equal(first, single[1])
    assert np.array_equal(v, single[2]) and np.array_equal(n, single[3])      # values: -0.0 + 0.0 is +0.0
    assert (rgba == np.array([9, 8, 7, 6], np.uint8)).all()
    mesh.destroy()
    sm.destroy()


def test_run_to_run_reuse_and_the_single_layer_calls(ctx):
    rng = np.random.default_rng(7)
    subs = _random_subs(rng, 8)
    handles = [capi.Submap(ctx, k, 0.2, 8, *s) for k, s in enumerate(subs)]
    T = np.stack([_general(rng, (0.3 * k, 0, 0)) for k in range(len(subs))])
    rgba = rng.integers(0, 256, (len(subs), 4), dtype=np.uint8)
    small = ([handles[2], handles[5]], T[[2, 5]], rgba[[2, 5]])
    fresh = _download(capi.Mesh(ctx).generate_separated(*small))
    m = capi.Mesh(ctx)
    m.generate_separated(handles, T, rgba)
    a = _download(m)
    m.generate_separated(handles, T, rgba)
    _assert_equal(_download(m), a)                                    # two identical calls
    m.generate_separated(*small)
    _assert_equal(_download(m), fresh)                                # a reused handle after a larger mesh
    # a single-layer mesh after a separated one: no colours, the fresh handle's mesh
    handles[1].generate_mesh(m)
    assert not m.has_colors()
    with pytest.raises(capi.VgxError) as e:
        m.download_colors()
    assert e.value.code == capi.ERR_INVALID
    want = handles[1].generate_mesh().download()
    for g, w in zip(m.download(), want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    layer = capi.TsdfLayer(ctx, 0.2, 8)
    layer.upload(*subs[0])
    m.generate_separated(*small)
    layer.generate_mesh(m)
    assert not m.has_colors()
    for g, w in zip(m.download(), layer.generate_mesh().download()):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    # n = 0 and only-empty submaps: 0 blocks... or the empty blocks, with colours
    m.generate_separated([], np.zeros((0, 7), F), np.zeros((0, 4), np.uint8))
    assert m.has_colors() and m.stats() == (0, 0) and m.download_colors().shape == (0, 4)
    m.generate_separated([handles[5]], T[5:6], rgba[5:6])
    assert m.has_colors() and m.stats() == (3, 0)
    assert m.download()[0].tolist() == [[0, 0, 0], [1, 0, 0], [5, 5, 5]]
    m.destroy()
    layer.destroy()
    for h in handles:
        h.destroy()


def test_refusals_leave_the_previous_mesh(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(11)
    data = edge_case_layer(rng, 8, (0, 0, 0), (2, 2, 2), density=1.0)
    a = capi.Submap(ctx, 1, 0.2, 8, *data)
    b = capi.Submap(ctx, 2, 0.2, 8, *data)
    T = np.stack([_yaw(0.2, (0, 0, 0)), _yaw(-0.4, (1, 0, 0))])
    rgba = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint8)
    m = capi.Mesh(ctx).generate_separated([a, b], T, rgba)
    before = _download(m)
    assert len(before[2]) > 0
    cfg = capi.MeshConfig(1e-4)
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)

    def call(c, subs, poses, colors, mesh, n=None, mcfg=cfg):
        arr = (C.c_void_p * max(len(subs), 1))(*[s if s is None else s.h for s in subs])
        p = None if poses is None else np.ascontiguousarray(poses, F).ctypes.data_as(f32p)
        q = None if colors is None else np.ascontiguousarray(colors, np.uint8).ctypes.data_as(u8p)
        return lib.vgx_submaps_generate_separated_mesh(c, len(subs) if n is None else n, arr, p, q, C.byref(mcfg), mesh)

    def refused(code, *args, say=None, **kw):
        assert call(*args, **kw) == code
        if say is not None:
            assert say in lib.vgx_last_error(ctx.h).decode()
        assert m.has_colors()
        _assert_equal(_download(m), before)

    I = capi.ERR_INVALID
    refused(I, None, [a, b], T, rgba, m.h)                                  # NULL ctx
    refused(I, ctx.h, [a, b], T, rgba, None, say="NULL mesh")
    other = capi.Context(0)
    m2 = capi.Mesh(other)
    refused(I, ctx.h, [a, b], T, rgba, m2.h, say="another context")          # a mesh of another context
    refused(I, ctx.h, [a, b], T, rgba, m.h, n=-1, say="n < 0")
    refused(I, ctx.h, [a, b], None, rgba, m.h, say="NULL")
    refused(I, ctx.h, [a, b], T, None, m.h, say="NULL")
    refused(I, ctx.h, [a, None], T, rgba, m.h, say="submap 1")
    c = capi.Submap(other, 3, 0.2, 8, *data)
    refused(I, ctx.h, [a, c], T, rgba, m.h, say="another context")          # a submap of another context
    d = capi.Submap(ctx, 4, 0.1, 8, *data)
    refused(I, ctx.h, [a, d], T, rgba, m.h, say="voxel_size")
    bi16 = np.array([[0, 0, 0]], np.int32)
    e16 = capi.Submap(ctx, 5, 0.2, 16, bi16, np.zeros((1, 4096), F), np.ones((1, 4096), F))
    refused(I, ctx.h, [a, e16], T, rgba, m.h, say="voxels_per_side")
    for bad in (np.nan, np.inf):
        Tb = T.copy()
        Tb[1, 5] = bad
        refused(I, ctx.h, [a, b], Tb, rgba, m.h, say="not finite")
    Tb = T.copy()
    Tb[1, :4] *= 1.001
    refused(I, ctx.h, [a, b], Tb, rgba, m.h, say="not unit")
    for bad in (-1.0, float("nan"), float("inf")):
        refused(I, ctx.h, [a, b], T, rgba, m.h, mcfg=capi.MeshConfig(bad), say="min_weight")
    # a union block box whose cells x n do not fit 64 bits
    far = [capi.Submap(ctx, 6 + k, 0.2, 8, np.array([[s * 2 ** 21] * 3], np.int32), data[1][:1], data[2][:1])
           for k, s in enumerate((-1, 1))]
    refused(capi.ERR_UNSUPPORTED, ctx.h, far, T, rgba, m.h, say="64-bit key")
    # a released raw layer
    b.release_raw_layers()
    refused(I, ctx.h, [a, b], T, rgba, m.h, say="released")
    assert call(ctx.h, [a, a], T, rgba, m.h, mcfg=capi.MeshConfig(1e-4)) == capi.OK
    assert lib.vgx_submaps_generate_separated_mesh(ctx.h, 1, (C.c_void_p * 1)(a.h), T.ctypes.data_as(f32p),
                                                   rgba.ctypes.data_as(u8p), None, m.h) == capi.OK   # NULL config
    for o in far + [a, b, c, d, e16]:
        o.destroy()
    m2.destroy()
    m.destroy()
    other.close()


def _parse_ply(raw, colored):
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode().split("\n")
    vdt = [("p", "<f4", 3), ("n", "<f4", 3)] + ([("c", "u1", 4)] if colored else [])
    T = int([h for h in header if h.startswith("element face ")][0].split()[-1])
    vert = np.frombuffer(raw[end:end + 3 * T * np.dtype(vdt).itemsize], np.dtype(vdt))
    faces = np.frombuffer(raw[end + len(vert.tobytes()):], np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    return header, vert.reshape(T, 3), faces


def test_ply_colored_and_uncolored(ctx, tmp_path):
    rng = np.random.default_rng(3)
    subs = [edge_case_layer(rng, 8, (-1, -1, 0), (3, 2, 2), density=1.0) for _ in range(2)]
    handles = [capi.Submap(ctx, k, 0.2, 8, *s) for k, s in enumerate(subs)]
    T = np.stack([_yaw(0.5, (0, 0, 0)), _general(rng, (0.3, 0.1, 0))])
    rgba = np.array([[200, 10, 30, 255], [0, 90, 250, 128]], np.uint8)
    m = capi.Mesh(ctx).generate_separated(handles, T, rgba)
    _, _, v, n, c = _download(m)
    path = tmp_path / "sep.ply"
    m.write_ply(str(path))
    header, vert, faces = _parse_ply(path.read_bytes(), True)
    props = [h for h in header if h.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property float nx", "property float ny",
                     "property float nz", "property uchar red", "property uchar green", "property uchar blue",
                     "property uchar alpha", "property list uchar int vertex_indices"]
    assert f"element vertex {3 * len(v)}" in header and len(v) > 0
    assert np.array_equal(vert["p"].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(vert["n"].view(np.uint32), np.repeat(n[:, None, :], 3, 1).view(np.uint32))
    assert np.array_equal(vert["c"], np.repeat(c[:, None, :], 3, 1))
    assert len(faces) == len(v) and np.array_equal(faces["i"].ravel(), np.arange(3 * len(v)))
    # uncoloured: the same handle after a single-layer mesh writes exactly what a never-coloured handle writes
    handles[0].generate_mesh(m)
    m.write_ply(str(tmp_path / "a.ply"))
    plain = handles[0].generate_mesh()
    plain.write_ply(str(tmp_path / "b.ply"))
    raw = (tmp_path / "a.ply").read_bytes()
    assert raw == (tmp_path / "b.ply").read_bytes() and b"uchar red" not in raw
    plain.destroy()
    m.destroy()
    for h in handles:
        h.destroy()


def test_city_scale_sample(ctx):
    """20 city submaps at 128^3 voxels along an overlapping trajectory: sampled output blocks against the restatement"""
    vs, vps = 0.1, 16
    n_sub = 20
    rng = np.random.default_rng(20)
    poses4 = [np.array([1.6 * k, 0.4 * np.sin(k), 0.05 * k, 0.15 * k]) for k in range(n_sub)]
    handles, data, T = [], [], []
    for k, p in enumerate(poses4):
        sm = capi.Submap.synth_city(ctx, k, vs, vps, (-4, -4, -4), (8, 8, 8), 0.3, 2.0, 10.0, p, 3)
        td, tw, _, _ = sm.download_layers(vps)
        data.append((sm.block_index(), td, tw))
        handles.append(sm)
        T.append(_yaw(p[3], p[:3]) if k % 2 else _general(rng, p[:3]))
    T = np.stack(T)
    rgba = np.stack([sr.submap_color(k) for k in range(n_sub)])
    mesh = capi.separated_mesh(ctx, handles, T)                      # IDs 0..19 in order: array order
    bi, first, v, n, c = _download(mesh)
    nb, nt = mesh.stats()
    assert nb == len(bi) and nt > 100000
    rows = [{tuple(x): i for i, x in enumerate(d[0].tolist())} for d in data]
    assert nb == len(set().union(*rows))
    with_tris = np.flatnonzero(np.diff(first) > 0)
    multi = [j for j in with_tris if sum(tuple(bi[j]) in r for r in rows) > 1]
    sample = list(rng.choice(with_tris, 24, replace=False)) + list(rng.choice(multi, 8, replace=False))
    offs = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    for j in sample:
        key = tuple(int(x) for x in bi[j])
        meshes, cols = [], []
        for s in range(n_sub):
            if key not in rows[s]:
                continue
            sel = [rows[s][k] for k in (tuple(a + o for a, o in zip(key, off)) for off in offs) if k in rows[s]]
            sub = (data[s][0][sel], data[s][1][sel], data[s][2][sel])    # the block and its +x/+y/+z neighbours
            m = sr.pose_mesh(mr.generate_mesh(*sub, vps, vs), T[s])
            k0 = [tuple(x) for x in m[0].tolist()].index(key)
            meshes.append((m[0][k0:k0 + 1], m[1][k0:k0 + 2] - m[1][k0], m[2][m[1][k0]:m[1][k0 + 1]], m[3][m[1][k0]:m[1][k0 + 1]]))
            cols.append(rgba[s])
        want = sr.combine(meshes, cols)
        got = (bi[j:j + 1], first[j:j + 2] - first[j], v[first[j]:first[j + 1]], n[first[j]:first[j + 1]],
               c[first[j]:first[j + 1]])
        _assert_equal(got, want)
    mesh.destroy()
    for h in handles:
        h.destroy()
