"""vgx_tsdf_layer_merge_submaps (the projected map, cblox::SubmapCollection::getProjectedMap) on the device, against the
numpy restatement of tests/projected_map_ref.py bit for bit, and against analytic scenes independently of it."""
import ctypes as C

import numpy as np
import pytest

from oracle import synth
from tests import projected_map_ref as pm
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
IDENT = np.array([1, 0, 0, 0, 0, 0, 0], F)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _yaw_pose(yaw, t):
    return np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)


def _quat_pose(axis, angle, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.array([np.cos(angle / 2), *(np.sin(angle / 2) * a), *t], F)


def _random_submap(rng, vps, vs, block_min, block_dims, density=1.0, zero_frac=0.05):
    bi = synth.dense_block_index(block_min, block_dims)
    if density < 1.0:
        bi = bi[rng.random(len(bi)) < density]
    n, nv = len(bi), vps ** 3
    d = rng.uniform(-0.3, 0.3, (n, nv)).astype(F)
    w = rng.uniform(0.5, 30, (n, nv)).astype(F)
    w[rng.random(w.shape) < zero_frac] = 0
    if n > 2:
        w[rng.integers(0, n)] = 0           # a block without data
    return type("Sm", (), dict(voxel_size=float(F(vs)), vps=vps, block_index=np.ascontiguousarray(bi, np.int32),
                               tsdf_distance=d, tsdf_weight=w))


def _upload(ctx, sm, sid):
    return capi.Submap(ctx, sid, sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight)


def _as_dict(layer):
    bi, d, w, rgba = layer.download()
    return {tuple(int(v) for v in b): (dd, ww) for b, dd, ww in zip(bi, d, w)}, bi, rgba


def _assert_layers_equal(got, want):
    assert set(got) == set(want), (len(set(got) ^ set(want)), sorted(set(got) ^ set(want))[:5])
    for k in want:
        gd, gw = got[k]
        wd, ww = want[k]
        assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (k, np.flatnonzero(gd.view(np.uint32) != wd.view(np.uint32))[:5])
        assert np.array_equal(gw.view(np.uint32), ww.view(np.uint32)), k


def _scene(vps):
    """6 overlapping submaps: dense and sparse block sets, identity / 4-DoF / 6-DoF poses"""
    rng = np.random.default_rng(vps)
    vs = 0.1 if vps == 16 else 0.2
    subs = [_random_submap(rng, vps, vs, (-2, -2, -1), (3, 3, 2)),
            _random_submap(rng, vps, vs, (-1, -2, -1), (3, 3, 2), density=0.5),
            _random_submap(rng, vps, vs, (-2, -1, 0), (3, 2, 2)),
            _random_submap(rng, vps, vs, (-3, -3, -1), (4, 4, 2), density=0.3),
            _random_submap(rng, vps, vs, (-1, -1, -1), (2, 2, 2)),
            _random_submap(rng, vps, vs, (-2, -2, -2), (3, 3, 3), density=0.7)]
    T = np.stack([IDENT, _yaw_pose(0.4, (0.37, -0.21, 0.05)), _quat_pose((0.3, -0.5, 0.8), 0.9, (0.1, 0.2, -0.3)),
                  _yaw_pose(-1.3, (0.0, 0.5, 0.0)), _quat_pose((1, 1, 0.2), -0.6, (-0.4, 0.3, 0.2)),
                  _yaw_pose(2.8, (0.05, 0.03, 0.11))])
    return subs, T


@pytest.mark.parametrize("vps", [16, 8])
def test_empty_layer_bit_exact(ctx, vps):
    subs, T = _scene(vps)
    handles = [_upload(ctx, s, i) for i, s in enumerate(subs)]
    layer = capi.TsdfLayer(ctx, subs[0].voxel_size, vps)
    nb = layer.merge_submaps(handles, T)
    got, bi, rgba = _as_dict(layer)
    want = pm.merge_submaps({}, subs, T)
    assert nb == len(got) == len(want) > 10
    _assert_layers_equal(got, want)
    assert not rgba.any()
    for h in handles:
        h.destroy()
    layer.destroy()


def test_non_empty_layer_bit_exact(ctx):
    subs, T = _scene(16)
    rng = np.random.default_rng(11)
    base = synth.dense_block_index((-2, -2, -1), (4, 3, 2))
    nv = 16 ** 3
    bd = rng.uniform(-0.3, 0.3, (len(base), nv)).astype(F)
    bw = rng.uniform(0, 8, (len(base), nv)).astype(F)
    bw[:, ::5] = 0
    rgba = rng.integers(0, 256, (len(base), nv, 4), dtype=np.uint8)
    layer = capi.TsdfLayer(ctx, subs[0].voxel_size, 16)
    layer.upload(base, bd, bw, rgba)
    handles = [_upload(ctx, s, i) for i, s in enumerate(subs)]
    layer.merge_submaps(handles, T)
    got, bi, grgba = _as_dict(layer)
    want = pm.merge_submaps(pm.layer_from_arrays(base, bd, bw), subs, T)
    _assert_layers_equal(got, want)
    slot = {tuple(int(v) for v in b): i for i, b in enumerate(bi)}
    for i, b in enumerate(base):
        assert np.array_equal(grgba[slot[tuple(int(v) for v in b)]], rgba[i])
    new = [slot[k] for k in got if k not in {tuple(int(v) for v in b) for b in base}]
    assert new and not grgba[new].any()
    for h in handles:
        h.destroy()
    layer.destroy()


def test_order(ctx):
    subs, T = _scene(8)
    handles = [_upload(ctx, s, 10 + i) for i, s in enumerate(subs)]
    fwd = capi.TsdfLayer(ctx, subs[0].voxel_size, 8)
    fwd.merge_submaps(handles, T)
    rev = capi.TsdfLayer(ctx, subs[0].voxel_size, 8)
    rev.merge_submaps(handles[::-1], T[::-1])
    g_fwd, g_rev = _as_dict(fwd)[0], _as_dict(rev)[0]
    _assert_layers_equal(g_rev, pm.merge_submaps({}, subs[::-1], T[::-1]))
    assert set(g_fwd) == set(g_rev)
    assert any(not np.array_equal(g_fwd[k][0], g_rev[k][0]) for k in g_fwd)   # f32 merge order shows in the last bits
    # projected_map: ID order whatever the input order
    outs = []
    for perm in ([0, 1, 2, 3, 4, 5], [5, 3, 1, 0, 2, 4], [2, 4, 0, 5, 1, 3]):
        layer = capi.TsdfLayer(ctx, subs[0].voxel_size, 8)
        capi.projected_map(ctx, [handles[i] for i in perm], T[perm], layer)
        outs.append(_as_dict(layer)[0])
        layer.destroy()
    for o in outs:
        _assert_layers_equal(o, g_fwd)
    for h in handles:
        h.destroy()
    fwd.destroy()
    rev.destroy()


def _sampled_submap(sdf64, T, vs, vps, block_min, block_dims, band, weight=10.0):
    """a submap whose voxel (centre c) holds the world SDF at T * c, evaluated in f64; weight only inside the band,
    distances unclamped there (no truncation inside the band)"""
    bi = synth.dense_block_index(block_min, block_dims)
    c = synth.voxel_centres(vs, vps, bi).astype(np.float64)
    q = np.asarray(T[:4], np.float64)
    q = q / np.linalg.norm(q)
    w0, u = q[0], q[1:]
    uv = 2 * np.cross(u, c)
    world = c + w0 * uv + np.cross(u, uv) + np.asarray(T[4:], np.float64)
    d = sdf64(world)
    w = np.where(np.abs(d) < band, weight, 0).astype(F)
    return type("Sm", (), dict(voxel_size=float(F(vs)), vps=vps, block_index=bi, tsdf_distance=d.astype(F), tsdf_weight=w))


def _world_check(ctx, sdf64, tol, vs=0.1, vps=16, band=0.4):
    poses = [_quat_pose((0.2, 0.9, 0.4), 0.5, (0.3, -0.2, 0.1)), _quat_pose((-0.7, 0.1, 0.6), -0.8, (-0.5, 0.4, 0.0)),
             _quat_pose((0.5, 0.5, -0.3), 1.9, (0.2, 0.1, -0.3))]
    subs = [_sampled_submap(sdf64, T, vs, vps, (-3, -3, -3), (6, 6, 6), band) for T in poses]
    handles = [_upload(ctx, s, i) for i, s in enumerate(subs)]
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.merge_submaps(handles, np.stack(poses))
    bi, d, w, _ = layer.download()
    c = synth.voxel_centres(vs, vps, bi).reshape(-1, 3).astype(np.float64)
    d, w = d.ravel(), w.ravel()
    truth = sdf64(c)
    # a voxel whose whole interpolation neighbourhood is inside the band in every submap: |sdf| < band - 2 voxels
    # (the neighbourhood lies within sqrt(3) voxels of the sample point)
    inner = (w > 0) & (np.abs(truth) < band - 2 * vs)
    for h in handles:
        h.destroy()
    layer.destroy()
    err = np.abs(d[inner] - truth[inner])
    assert inner.sum() > 3000, inner.sum()
    return err, tol


def test_world_sdf_plane(ctx):
    """trilinear interpolation of a linear field is exact up to rounding: catches T vs T^-1"""
    n = np.array([0.3, -0.5, 0.81])
    n = n / np.linalg.norm(n)
    err, tol = _world_check(ctx, lambda p: p @ n - 0.2, 1e-5)
    assert err.max() < tol, err.max()


def test_world_sdf_sphere(ctx):
    """sphere of radius R: the SDF's Hessian has norm 1/r, so trilinear interpolation errs by at most
    3 h^2 / (8 r) per voxel of size h; with r >= R - band = 1.6 m and h = 0.1 m that is 2.4 mm"""
    centre, R = np.array([0.1, -0.2, 0.15]), 2.0
    err, tol = _world_check(ctx, lambda p: np.linalg.norm(p - centre, axis=-1) - R, 3 * 0.1 ** 2 / (8 * 1.6) + 1e-5)
    assert err.max() < tol, err.max()


def test_sources_may_go_right_after_the_call(ctx):
    subs, T = _scene(16)
    handles = [_upload(ctx, s, i) for i, s in enumerate(subs)]
    extra = _upload(ctx, subs[0], 99)
    layer = capi.TsdfLayer(ctx, subs[0].voxel_size, 16)
    layer.merge_submaps(handles, T)
    for h in handles:
        h.destroy()
    extra.release_raw_layers()
    _assert_layers_equal(_as_dict(layer)[0], pm.merge_submaps({}, subs, T))
    extra.destroy()
    layer.destroy()


def test_errors_leave_the_layer_untouched(ctx):
    rng = np.random.default_rng(7)
    s16 = _random_submap(rng, 16, 0.1, (-1, -1, -1), (2, 2, 2))
    s8 = _random_submap(rng, 8, 0.1, (-1, -1, -1), (2, 2, 2))
    s_vs = _random_submap(rng, 16, 0.2, (-1, -1, -1), (2, 2, 2))
    ok, wrong_vps, wrong_vs, released = (_upload(ctx, s16, 0), _upload(ctx, s8, 1), _upload(ctx, s_vs, 2),
                                         _upload(ctx, s16, 3))
    released.release_raw_layers()
    layer = capi.TsdfLayer(ctx, 0.1, 16)
    base = synth.dense_block_index((0, 0, 0), (2, 1, 1))
    bd = rng.uniform(-1, 1, (2, 4096)).astype(F)
    bw = rng.uniform(0, 1, (2, 4096)).astype(F)
    layer.upload(base, bd, bw)
    before = layer.download()

    def refused(subs, T):
        with pytest.raises(capi.VgxError) as e:
            layer.merge_submaps(subs, T)
        assert e.value.code == capi.ERR_INVALID, e.value
        after = layer.download()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        return str(e.value)

    assert "voxels_per_side" in refused([ok, wrong_vps], [IDENT, IDENT])
    assert "voxel_size" in refused([wrong_vs], [IDENT])
    assert "released" in refused([ok, released], [IDENT, IDENT])
    for bad in (np.nan, np.inf):
        T = IDENT.copy()
        T[5] = bad
        assert "finite" in refused([ok], [T])
    assert "unit" in refused([ok], [np.array([1.001, 0, 0, 0, 0, 0, 0], F)])
    assert "unit" in refused([ok], [np.array([0.5, 0.5, 0.5, 0.4, 0, 0, 0], F)])
    lib = ctx.lib
    nb = C.c_int64()
    assert lib.vgx_tsdf_layer_merge_submaps(layer.h, -1, None, None, C.byref(nb)) == capi.ERR_INVALID
    assert lib.vgx_tsdf_layer_merge_submaps(layer.h, 1, None, None, C.byref(nb)) == capi.ERR_INVALID
    assert all(np.array_equal(a, b) for a, b in zip(before, layer.download()))
    assert lib.vgx_tsdf_layer_merge_submaps(layer.h, 0, None, None, C.byref(nb)) == capi.OK and nb.value == 2
    assert all(np.array_equal(a, b) for a, b in zip(before, layer.download()))
    # a quaternion within the tolerance is accepted
    layer.merge_submaps([ok], [np.array([1.00004, 0, 0, 0, 0, 0, 0], F)])
    for h in (ok, wrong_vps, wrong_vs, released):
        h.destroy()
    layer.destroy()


def test_city_scale(ctx):
    """20 city submaps at 128^3 voxels along an overlapping trajectory: sampled target blocks and every block of one
    two-submap overlap against the restatement"""
    vs, vps = 0.1, 16
    n_sub = 20
    rng = np.random.default_rng(20)
    poses4 = [np.array([1.6 * k, 0.4 * np.sin(k), 0.05 * k, 0.15 * k]) for k in range(n_sub)]
    handles, subs, T = [], [], []
    for k, p in enumerate(poses4):
        sm = capi.Submap.synth_city(ctx, k, vs, vps, (-4, -4, -4), (8, 8, 8), 0.3, 2.0, 10.0, p, 3)
        td, tw, _, _ = sm.download_layers(vps)
        subs.append(type("Sm", (), dict(voxel_size=float(F(vs)), vps=vps, block_index=sm.block_index(),
                                        tsdf_distance=td, tsdf_weight=tw)))
        handles.append(sm)
        T.append(_yaw_pose(p[3], p[:3]))
    T = np.stack(T)
    layer = capi.TsdfLayer(ctx, vs, vps)
    capi.projected_map(ctx, handles, T, layer)
    got = _as_dict(layer)[0]
    keys = sorted(got)
    sample = [keys[i] for i in rng.choice(len(keys), 64, replace=False)]
    want = pm.merge_submaps({}, subs, T, only=np.array(sample))
    for k in sample:
        assert k in want
    _assert_layers_equal({k: got[k] for k in want}, want)
    # every block of the overlap of submaps 6 and 7 (alone: the other submaps do not reach all of them)
    pair = capi.TsdfLayer(ctx, vs, vps)
    pair.merge_submaps(handles[6:8], T[6:8])
    _assert_layers_equal(_as_dict(pair)[0], pm.merge_submaps({}, subs[6:8], T[6:8]))
    for h in handles:
        h.destroy()
    layer.destroy()
    pair.destroy()
