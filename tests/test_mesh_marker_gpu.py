"""vgx_mesh_fill_marker (voxblox_ros fillMarkerWithMesh) on the device: bit for bit against the numpy restatement of
tests/mesh_marker_ref.py through the C ABI -- every mode on layer meshes with an odd triangle count at vps 8 and 16, one
cube, the empty layer, the HEIGHT column, a separated mesh with colours, a constant colour, the opacity, a reused handle
going large, small, large, run to run, the device pointers, every refusal and the untouched source.
Not provoked here: the refusal of a source handle whose last generating call failed (an allocation or device failure
sets the flag behind it), 3 T >= 2^32 (1.4 G triangles) and out of device memory."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import mesh_marker_ref as R
from tests.test_mesh_cpu import edge_case_layer
from tests.test_mesh_marker_cpu import height_layer
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _want(mesh, mode, opacity=1.0, constant_rgba=None):
    _, _, v, n = mesh.download()
    colors = mesh.download_colors() if mesh.has_colors() else None
    return R.fill_marker(v, n, colors, mode, opacity, constant_rgba)


def _assert_equal(got, want):
    for name, g, w in zip(("points", "colors"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())
        assert len(bad) == 0, (name, len(bad), bad[:5])


def _check(mesh, mode, out, opacity=1.0, constant_rgba=None):
    capi.fill_marker(mesh, mode, opacity, constant_rgba, out)
    want = _want(mesh, mode, opacity, constant_rgba)
    assert out.stats() == (3 * mesh.stats()[1], mode)
    got = out.download()
    _assert_equal(got, want)
    return got


# seeds at which the layer's mesh has an odd triangle count (asserted): 72 T and 9 T are then no multiples of 16 and 2
@pytest.mark.parametrize("vps,seed", [(8, 3), (16, 0)])
def test_every_mode_on_a_layer_mesh_bit_exact(ctx, vps, seed):
    rng = np.random.default_rng(seed)
    vs = 0.2 if vps == 8 else 0.1
    data = edge_case_layer(rng, vps, (-2, -1, -1), (2, 2, 2))
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.upload(*data)
    mesh = layer.generate_mesh()
    src_before = mesh.download()
    T = mesh.stats()[1]
    assert T % 2 == 1 and T > 2000 and T % 256 != 0, T
    assert (np.abs(src_before[3]).sum(1) == 0).any()                 # degenerate triangles with a zero normal
    out = capi.MeshMarker(ctx)
    seen = []
    for mode in (R.HEIGHT, R.NORMALS, R.GRAY, R.LAMBERT):
        seen.append(_check(mesh, mode, out, opacity=0.25)[1])
        assert (seen[-1][:, 3] == F(0.25)).all()                     # the opacity lands in every alpha
    const = (200, 30, 255, 9)
    for mode in (R.COLOR, R.LAMBERT_COLOR):                          # a mesh without colours: the constant colour
        seen.append(_check(mesh, mode, out, opacity=0.25, constant_rgba=const)[1])
    assert (seen[4][:, :3] == R.C8[list(const[:3])]).all()
    assert len({c.tobytes() for c in seen}) == len(seen)             # the modes differ
    for g, s in zip(mesh.download(), src_before):                    # the source is not changed
        assert np.array_equal(g.view(np.uint8), s.view(np.uint8))
    assert not mesh.has_colors()
    for o in (out, mesh, layer):
        o.destroy()


def _one_cube_layer(vps=8):
    d = np.full((1, vps ** 3), 0.1, F)
    w = np.zeros((1, vps ** 3), F)
    for x in (3, 4):
        for y in (3, 4):
            for z in (3, 4):
                w[0, x + vps * (y + vps * z)] = 1
    d[0, 3 + vps * (3 + vps * 3)] = -0.07
    d[0, 4 + vps * (3 + vps * 3)] = -0.02
    return np.array([[1, -2, 0]], np.int32), d, w


def test_one_cube_empty_layer_and_height_column(ctx):
    out = capi.MeshMarker(ctx)
    layer = capi.TsdfLayer(ctx, 0.1, 8)
    layer.upload(*_one_cube_layer())
    mesh = layer.generate_mesh()
    assert 1 <= mesh.stats()[1] <= 5
    for mode in (R.HEIGHT, R.NORMALS, R.GRAY, R.LAMBERT):
        _check(mesh, mode, out)
    _check(mesh, R.LAMBERT_COLOR, out, constant_rgba=(255, 255, 255, 255))
    # an empty layer (no blocks), and a mesh handle never filled: VGX_OK and 0 points
    layer.upload(np.zeros((0, 3), np.int32), np.zeros((0, 512), F), np.zeros((0, 512), F))
    layer.generate_mesh(mesh)
    assert mesh.stats() == (0, 0)
    for m in (mesh, capi.Mesh(ctx)):
        capi.fill_marker(m, R.NORMALS, out=out)
        assert out.stats() == (0, R.NORMALS) and out.device_pointers() == (None, None)
        assert [a.shape for a in out.download()] == [(0, 3), (0, 4)]
    # HEIGHT over the column of blocks: all six sectors and both clamps (tests/test_mesh_marker_cpu.py shows it)
    vs, vps, data = height_layer()
    column = capi.TsdfLayer(ctx, vs, vps)
    column.upload(*data)
    column.generate_mesh(mesh)
    got = _check(mesh, R.HEIGHT, out)
    z = got[0][:, 2].astype(F)
    inside = (z > -1) & (z < 10)
    assert z.min() < -1.5 and z.max() > 10.5                         # both clamps, on the device's own mesh
    assert sorted(set(R.rainbow_sector(R.height_ratio(z[inside])).tolist())) == [0, 1, 2, 3, 4, 5]
    for o in (out, mesh, layer, column):
        o.destroy()


def _yaw(yaw, t):
    return np.array([math.cos(yaw / 2), 0, 0, math.sin(yaw / 2), *t], F)


def test_separated_mesh_colours_follow_the_triangles(ctx):
    rng = np.random.default_rng(4)
    subs = [edge_case_layer(rng, 8, (-1 + k % 2, -1, -1), (2, 2, 2), density=0.9) for k in range(3)]
    handles = [capi.Submap(ctx, k, 0.2, 8, *s) for k, s in enumerate(subs)]
    T = np.stack([_yaw(0.2 * k - 0.3, (0.4 * k, -0.2 * k, 0.1)) for k in range(3)])
    rgba = np.array([[255, 10, 0, 255], [0, 128, 255, 40], [77, 255, 127, 0]], np.uint8)
    mesh = capi.Mesh(ctx).generate_separated(handles, T, rgba)
    _, first, _, _ = mesh.download()
    colors = mesh.download_colors()
    # shared block indices: an output block holds triangles of several submaps
    assert sum(len(np.unique(colors[first[k]:first[k + 1]], axis=0)) > 1 for k in range(len(first) - 1)) > 3
    out = capi.MeshMarker(ctx)
    got = _check(mesh, R.COLOR, out)
    assert np.array_equal(got[1][:, :3], np.repeat(R.C8[colors[:, :3]], 3, 0)) and (got[1][:, 3] == 1).all()
    assert len(np.unique(got[1], axis=0)) == 3
    lam = _check(mesh, R.LAMBERT_COLOR, out, opacity=0.5)
    assert not np.array_equal(lam[1][:, :3], got[1][:, :3])
    # the constant colour wins over the mesh's colours; LAMBERT ignores both
    const = (9, 99, 199, 255)
    a = _check(mesh, R.LAMBERT_COLOR, out, constant_rgba=const)
    _, _, v, n = mesh.download()
    _assert_equal(a, R.fill_marker(v, n, np.tile(np.array(const, np.uint8), (len(v), 1)), R.LAMBERT_COLOR))
    _check(mesh, R.LAMBERT, out, constant_rgba=const)
    _assert_equal(out.download(), R.fill_marker(v, n, None, R.LAMBERT))
    for o in (out, mesh, *handles):
        o.destroy()


def test_reuse_runs_and_device_pointers(ctx):
    import torch
    rng = np.random.default_rng(9)
    big_sm = capi.Submap(ctx, 1, 0.2, 8, *edge_case_layer(rng, 8, (-1, -2, 0), (3, 3, 2)))
    small_sm = capi.Submap(ctx, 2, 0.2, 8, *edge_case_layer(rng, 8, (0, 0, 0), (2, 1, 1), density=1.0))
    big, sml = big_sm.generate_mesh(), small_sm.generate_mesh()
    assert big.stats()[1] > 4 * sml.stats()[1] > 400
    out = capi.MeshMarker(ctx)
    a = _check(big, R.LAMBERT, out)                                  # large
    capi.fill_marker(big, R.LAMBERT, out=out)
    _assert_equal(out.download(), a)                                 # two runs, the same bytes
    fresh = capi.fill_marker(sml, R.NORMALS)
    _assert_equal(_check(sml, R.NORMALS, out), fresh.download())     # small
    _assert_equal(_check(big, R.LAMBERT, out), a)                    # large again
    # the device arrays, read through torch, are the download
    n, _ = out.stats()
    dp, dc = out.device_pointers()
    assert n > 0 and dp and dc

    class Wrapped:                                                   # (torch and the library share one HIP runtime)
        def __init__(self, ptr, shape, typestr):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2,
                                             "strides": None}

    p = torch.as_tensor(Wrapped(dp, (n, 3), "<f8"), device="cuda:0")
    c = torch.as_tensor(Wrapped(dc, (n, 4), "<f4"), device="cuda:0")
    assert p.dtype == torch.float64 and c.dtype == torch.float32
    _assert_equal((p.cpu().numpy(), c.cpu().numpy()), a)
    del p, c
    for o in (fresh, out, big, sml, big_sm, small_sm):
        o.destroy()


def test_refusals(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(11)
    sm = capi.Submap(ctx, 1, 0.2, 8, *edge_case_layer(rng, 8, (0, 0, 0), (2, 2, 1), density=1.0))
    mesh = sm.generate_mesh()
    src_before = mesh.download()
    out = capi.MeshMarker(ctx)
    before = _check(mesh, R.NORMALS, out, opacity=0.5)
    assert len(before[0]) > 300

    def refused(code, m, cfg, o, say):
        assert lib.vgx_mesh_fill_marker(m, None if cfg is None else C.byref(cfg), o) == code
        assert say in lib.vgx_last_error(ctx.h).decode(), lib.vgx_last_error(ctx.h).decode()
        assert out.stats() == (len(before[0]), R.NORMALS)            # refused before anything is written
        _assert_equal(out.download(), before)

    I = capi.ERR_INVALID
    ok = capi.mesh_marker_config(color_mode=R.GRAY)
    refused(I, None, ok, out.h, "NULL mesh")
    refused(I, mesh.h, ok, None, "NULL marker")
    other = capi.Context(0)
    out2 = capi.MeshMarker(other)
    refused(I, mesh.h, ok, out2.h, "another context")
    for mode in (-1, 6, 1 << 20):
        refused(I, mesh.h, capi.mesh_marker_config(color_mode=mode), out.h, "color_mode")
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(I, mesh.h, capi.mesh_marker_config(color_mode=R.GRAY, opacity=bad), out.h, "opacity")
    for mode in (R.COLOR, R.LAMBERT_COLOR):                          # voxblox CHECKs hasColors()
        refused(I, mesh.h, capi.mesh_marker_config(color_mode=mode), out.h, "no colours")
    refused(I, mesh.h, None, out.h, "no colours")                    # NULL cfg: the defaults, LAMBERT_COLOR
    # the same modes pass with a constant colour, and on a mesh with colours NULL cfg is LAMBERT_COLOR at opacity 1
    _check(mesh, R.COLOR, out, constant_rgba=(1, 2, 3, 4))
    colored = capi.Mesh(ctx).generate_separated([sm], _yaw(0.1, (0, 0, 0))[None], np.array([[250, 128, 3, 4]], np.uint8))
    ctx.check(lib.vgx_mesh_fill_marker(colored.h, None, out.h))
    assert out.stats()[1] == R.LAMBERT_COLOR
    _assert_equal(out.download(), _want(colored, R.LAMBERT_COLOR, 1.0))
    for g, s in zip(mesh.download(), src_before):                    # the source is not changed
        assert np.array_equal(g.view(np.uint8), s.view(np.uint8))
    for o in (out2, out, colored, mesh, sm):
        o.destroy()
    other.close()
