"""Map queries on the device: vgx_submap_query / _device (voxblox's EsdfMap / TsdfMap lookups) against the numpy
restatement of tests/map_query_ref.py bit for bit -- both layers, vps 8 and 16, every interpolate / gradient combination,
with and without a pose, shuffled slot orders, points near the surface, in free space, outside the map and on block
boundaries, the window route and its fallback, the host and device calls, the projected map made queryable, 10^6 points
on a 256^3 city submap -- and every refusal."""
import numpy as np
import pytest

from oracle import synth
from tests import map_query_ref as R
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
MODES = [(False, False), (True, False), (False, True), (True, True)]  # (interpolate, gradient)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _yaw_pose(yaw, t):
    return np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)


def _full_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.array([*q, *rng.uniform(-1, 1, 3)], F)


def _random_submap(rng, vps, vs=0.1, shuffle=True):
    """a block set with holes, shuffled slot order; ESDF and TSDF values random, ~10 % unobserved / zero weight"""
    pool = synth.dense_block_index((-3, -2, -2), (6, 4, 4))
    bi = pool[rng.random(len(pool)) < 0.8]
    if shuffle:
        bi = bi[rng.permutation(len(bi))]
    n, nv = len(bi), vps ** 3
    td = rng.uniform(-0.3, 0.3, (n, nv)).astype(F)
    tw = np.where(rng.random((n, nv)) < 0.1, F(0), rng.uniform(0.1, 10, (n, nv)).astype(F)).astype(F)
    ed = rng.uniform(-1, 3, (n, nv)).astype(F)
    eo = (rng.random((n, nv)) < 0.9).astype(np.uint8)
    return synth.SubmapData(vs, vps, bi.astype(np.int32), td, tw, ed, eo, np.zeros(4))


def _upload(ctx, sid, d):
    return capi.Submap(ctx, sid, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.esdf_distance,
                       d.esdf_observed)


def _points(rng, d, n):
    """inside the blocks, outside the map, on block faces and voxel centres / faces"""
    vs, bs = F(d.voxel_size), F(d.voxel_size * d.vps)
    lo = d.block_index.min(0) * bs
    hi = (d.block_index.max(0) + 1) * bs
    inside = rng.uniform(lo, hi, (n, 3)).astype(F)
    outside = rng.uniform(lo - 2 * bs, hi + 2 * bs, (n // 4, 3)).astype(F)
    faces = rng.uniform(lo, hi, (n // 4, 3)).astype(F)
    ax = rng.integers(0, 3, len(faces))
    faces[np.arange(len(faces)), ax] = (np.round(faces[np.arange(len(faces)), ax] / bs) * bs).astype(F)
    grid = (np.floor(rng.uniform(lo, hi, (n // 4, 3)) / vs) * vs + rng.choice([0.0, 0.5], (n // 4, 3)) * vs).astype(F)
    return np.concatenate([inside, outside, faces, grid]).astype(F)


def _check(ctx, sm, d, p, layer, interp, grad, pose=None):
    got = sm.query(p, layer, interpolate=interp, gradient=grad, pose=pose, weight=layer == "tsdf")
    wd, wg, ww, wok = R.query(d, p, layer, interpolate=interp, gradient=grad, pose=pose)
    assert np.array_equal(got.valid, wok), (layer, interp, grad, int((got.valid != wok).sum()))
    assert np.array_equal(_bits(got.distance), _bits(wd)), (layer, interp, grad)
    if grad:
        assert np.array_equal(_bits(got.gradient), _bits(wg)), (layer, interp, grad)
    else:
        assert got.gradient is None
    if layer == "tsdf":
        assert np.array_equal(_bits(got.weight), _bits(ww))
    return got


@pytest.mark.parametrize("vps", [8, 16])
@pytest.mark.parametrize("layer", ["esdf", "tsdf"])
def test_query_bit_exact(ctx, vps, layer):
    rng = np.random.default_rng(vps * 10 + (layer == "tsdf"))
    d = _random_submap(rng, vps)
    sm = _upload(ctx, 1, d)
    p = _points(rng, d, 4000)
    for pose in (None, _yaw_pose(0.7, (0.3, -0.2, 0.1)), _full_pose(rng)):
        q = p if pose is None else R.quat_rotate(pose[:4], p) + pose[4:]  # the same points seen from frame Q
        for interp, grad in MODES:
            got = _check(ctx, sm, d, q.astype(F), layer, interp, grad, pose)
            assert got.valid.any() and not got.valid.all()
    sm.destroy()


def test_query_on_a_city_submap_near_surface_and_free_space(ctx):
    rng = np.random.default_rng(5)
    vs, vps = 0.1, 16
    sm = capi.Submap.synth_city(ctx, 0, vs, vps, (-2, -2, -1), (4, 4, 2), 0.3, 2.0, 10.0, np.array([0.1, 0.2, 0.0, 0.3]), 3)
    td, tw, ed, eo = sm.download_layers(vps)
    d = synth.SubmapData(float(F(vs)), vps, sm.block_index(), td, tw, ed, eo, np.zeros(4))
    assert sm.extract_isosurface_points() > 0
    xyz = sm.download_points(capi.POINTS_ISOSURFACE)[0]
    near = (xyz[rng.integers(0, len(xyz), 3000)] + rng.normal(0, 0.05, (3000, 3))).astype(F)
    free = rng.uniform((-3.2, -3.2, -1.6), (3.2, 3.2, 1.6), (3000, 3)).astype(F)
    for layer in ("esdf", "tsdf"):
        for interp, grad in MODES:
            _check(ctx, sm, d, near, layer, interp, grad)
            _check(ctx, sm, d, free, layer, interp, grad, _yaw_pose(-0.2, (0.05, 0.1, 0.0)))
    sm.destroy()


@pytest.mark.parametrize("vps", [8, 16])
def test_window_route_and_its_fallback(ctx, vps):
    """dense points everywhere in a fully observed map (the window route) and, where a gradient offset's low neighbour
    is not G0 +- e_a (points a hair off voxel centres, where p +- voxel_size rounds across a centre), the generic route"""
    rng = np.random.default_rng(11 + vps)
    d = _random_submap(rng, vps, vs=0.1, shuffle=True)
    d.esdf_observed[:] = 1
    d.tsdf_weight[:] = np.maximum(d.tsdf_weight, F(0.5))
    sm = _upload(ctx, 2, d)
    bs = F(0.1 * vps)
    lo, hi = d.block_index.min(0) * bs, (d.block_index.max(0) + 1) * bs
    dense = rng.uniform(lo, hi, (60000, 3)).astype(F)
    c = ((np.floor(rng.uniform(lo, hi, (20000, 3)) / F(0.1)) + F(0.5)) * F(0.1)).astype(F)
    off = (c + rng.choice([-1, 0, 1], c.shape) * np.spacing(c)).astype(F)
    p = np.concatenate([dense, c, off])
    for layer in ("esdf", "tsdf"):
        got = _check(ctx, sm, d, p, layer, True, True)
        assert got.valid.mean() > 0.3  # (a fifth of the blocks are missing)
    sm.destroy()


def test_host_and_device_calls_agree(ctx):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(21)
    d = _random_submap(rng, 16)
    sm = _upload(ctx, 3, d)
    p = _points(rng, d, 20000)
    tp = torch.from_numpy(p).to("cuda:0")
    for layer in ("esdf", "tsdf"):
        for interp, grad in MODES:
            for pose in (None, _full_pose(rng)):
                h = sm.query(p, layer, interp, grad, pose, weight=layer == "tsdf")
                g = sm.query_device(tp, layer, interp, grad, pose, weight=layer == "tsdf")
                assert np.array_equal(h.valid.view(np.uint8), g.valid.cpu().numpy())
                assert np.array_equal(_bits(h.distance), _bits(g.distance.cpu().numpy()))
                if grad:
                    assert np.array_equal(_bits(h.gradient), _bits(g.gradient.cpu().numpy()))
                if layer == "tsdf":
                    assert np.array_equal(_bits(h.weight), _bits(g.weight.cpu().numpy()))
    # asynchronous form: queued on the registration stream, complete after ctx.synchronize()
    g = sm.query_device(tp, "esdf", True, True, sync=False)
    ctx.synchronize()
    h = sm.query(p, "esdf", True, True)
    assert np.array_equal(_bits(h.gradient), _bits(g.gradient.cpu().numpy()))
    sm.destroy()


def test_projected_map_becomes_queryable(ctx):
    """vgx_tsdf_layer_merge_submaps, vgx_submap_from_tsdf_layer, vgx_submap_generate_esdf, then the query"""
    rng = np.random.default_rng(31)
    vs, vps = 0.1, 16
    poses = [np.array([1.6 * k, 0.3 * np.sin(k), 0.03 * k, 0.1 * k]) for k in range(3)]
    subs = [capi.Submap.synth_city(ctx, k, vs, vps, (-2, -2, -1), (4, 4, 2), 0.3, 2.0, 10.0, p, 3)
            for k, p in enumerate(poses)]
    layer = capi.TsdfLayer(ctx, vs, vps)
    capi.projected_map(ctx, subs, np.stack([_yaw_pose(p[3], p[:3]) for p in poses]), layer)
    pm = capi.Submap.from_tsdf_layer(ctx, layer, 50)
    pm.generate_esdf()
    td, tw, ed, eo = pm.download_layers(vps)
    d = synth.SubmapData(float(F(vs)), vps, pm.block_index(), td, tw, ed, eo, np.zeros(4))
    p = rng.uniform((-3, -3.5, -1.5), (6.5, 3.5, 1.5), (20000, 3)).astype(F)
    for lay in ("esdf", "tsdf"):
        for interp, grad in MODES:
            got = _check(ctx, pm, d, p, lay, interp, grad)
            assert got.valid.any()
    pm.destroy()
    layer.destroy()
    for s in subs:
        s.destroy()


def test_a_million_points_on_a_256_cube_city_submap(ctx):
    rng = np.random.default_rng(41)
    vs, vps = 0.1, 16
    sm = capi.Submap.synth_city(ctx, 0, vs, vps, (-8, -8, -8), (16, 16, 16), 0.3, 2.0, 10.0, np.array([0.0, 0.0, 0.0, 0.1]), 7)
    td, tw, ed, eo = sm.download_layers(vps)
    d = synth.SubmapData(float(F(vs)), vps, sm.block_index(), td, tw, ed, eo, np.zeros(4))
    p = rng.uniform(-13.5, 13.5, (1_000_000, 3)).astype(F)
    got = _check(ctx, sm, d, p, "esdf", True, True, _yaw_pose(0.4, (0.2, -0.1, 0.05)))
    assert got.valid.mean() > 0.1  # (the city's ESDF is observed up to 2 m from the surface)
    sm.destroy()


def test_refusals_and_empty_queries(ctx):
    rng = np.random.default_rng(51)
    d = _random_submap(rng, 8)
    sm = _upload(ctx, 4, d)
    lib = ctx.lib
    n = 4
    p = np.zeros((n, 3), F)
    dist = np.full(n, 7.0, F)
    grad = np.full((n, 3), 7.0, F)
    wgt = np.full(n, 7.0, F)
    val = np.full(n, 9, np.uint8)
    f32 = lambda a: None if a is None else a.ctypes.data_as(capi.f32p)  # noqa: E731
    u8 = lambda a: None if a is None else a.ctypes.data_as(capi.u8p)  # noqa: E731

    def rc(h=sm.h, layer=0, flags=1, T=None, n=n, p=p, d=dist, g=None, w=None, v=val):
        return lib.vgx_submap_query(h, layer, flags, f32(T), n, f32(p), f32(d), f32(g), f32(w), u8(v))

    bad = [
        dict(h=None), dict(n=-1), dict(p=None), dict(d=None), dict(v=None), dict(flags=2), dict(flags=4), dict(flags=-1),
        dict(layer=2), dict(layer=-1), dict(w=wgt), dict(T=np.array([1, 0, 0, 0, np.nan, 0, 0], F)),
        dict(T=np.array([1.1, 0, 0, 0, 0, 0, 0], F)), dict(T=np.array([np.inf, 0, 0, 0, 0, 0, 0], F)),
    ]
    for kw in bad:
        assert rc(**kw) == capi.ERR_INVALID, kw
        assert (dist == 7).all() and (val == 9).all() and (grad == 7).all() and (wgt == 7).all(), kw
    assert lib.vgx_submap_query_device(sm.h, 0, 2, None, n, None, None, None, None, None) == capi.ERR_INVALID
    assert rc(n=0, p=None, d=None, v=None) == capi.OK
    assert rc(n=0, p=None, d=None, v=None, layer=1, flags=3, g=grad, w=wgt) == capi.OK
    assert lib.vgx_submap_query_device(sm.h, 1, 3, None, 0, None, None, None, None, None) == capi.ERR_INVALID  # no gradient
    assert lib.vgx_submap_query_device(sm.h, 1, 1, None, 0, None, None, None, None, None) == capi.OK
    assert (dist == 7).all() and (val == 9).all()
    assert rc(layer=1, flags=3, g=grad, w=wgt) == capi.OK  # and the same call with good arguments runs
    # a submap without a block, with and without a pose, every route: every query invalid, every output zero
    none = capi.Submap(ctx, 6, d.voxel_size, d.vps, np.zeros((0, 3), np.int32), np.zeros((0, d.vps ** 3), F),
                       np.zeros((0, d.vps ** 3), F))
    near = rng.uniform(-1, 1, (n, 3)).astype(F)
    turn = np.array([np.cos(0.4), 0, np.sin(0.4), 0, 0.3, -0.2, 0.1], F)
    for T in (None, turn):
        for layer, flags in ((0, 0), (0, 1), (0, 3), (1, 0), (1, 1), (1, 3)):
            for a, fill in ((dist, 7.0), (grad, 7.0), (wgt, 7.0), (val, 9)):
                a[...] = fill
            assert rc(h=none.h, layer=layer, flags=flags, T=T, p=near, g=grad if flags & 2 else None, w=wgt if layer else None) == capi.OK
            assert not dist.any() and not val.any(), (layer, flags)
            assert not grad.any() if flags & 2 else (grad == 7).all()
            assert not wgt.any() if layer else (wgt == 7).all()
    none.destroy()
    # a released raw layer, an ESDF never generated
    sm.release_raw_layers()
    assert rc() == capi.ERR_INVALID and rc(layer=1) == capi.ERR_INVALID
    sm.destroy()
    no_esdf = capi.Submap(ctx, 5, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight)
    assert rc(h=no_esdf.h) == capi.ERR_INVALID
    assert rc(h=no_esdf.h, layer=1) == capi.OK
    with pytest.raises(capi.VgxError):
        no_esdf.query(p, "esdf")
    no_esdf.destroy()
