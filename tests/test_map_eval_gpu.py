"""Map evaluation on the device: vgx_tsdf_layer_transform_submap (voxblox transformLayer) and vgx_evaluate_layers_rmse
(evaluateLayersRmse) against the numpy restatement of tests/map_eval_ref.py bit for bit, their refusals, and
capi.map_evaluation (MapEvaluation::evaluate) end to end with the harness solver doing the alignment."""
import ctypes as C

import numpy as np
import pytest

from oracle import synth
from tests import map_eval_ref as R
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("num_evaluated_voxels", "num_ignored_voxels", "num_overlapping_voxels", "num_non_overlapping_voxels")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _yaw_pose(yaw, t):
    return np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _esdf_pair(rng, vps, n_common, n_gt_only, n_test_only, shuffle=True):
    """gt and test ESDF layers on partially overlapping block sets, in shuffled slot orders"""
    pool = synth.dense_block_index((-4, -4, -2), (8, 8, 4))
    pick = rng.choice(len(pool), n_common + n_gt_only + n_test_only, replace=False)
    common, g_only, t_only = np.split(pool[pick], [n_common, n_common + n_gt_only])
    gbi, tbi = np.concatenate([common, g_only]), np.concatenate([common, t_only])
    if shuffle:
        gbi, tbi = gbi[rng.permutation(len(gbi))], tbi[rng.permutation(len(tbi))]
    nv = vps ** 3

    def layer(n):
        d = rng.uniform(-1.0, 2.0, (n, nv)).astype(F)
        o = (rng.random((n, nv)) < 0.85).astype(np.uint8)
        w = np.where(rng.random((n, nv)) < 0.15, F(0), rng.uniform(0.0, 5.0, (n, nv)).astype(F)).astype(F)
        w[rng.random((n, nv)) < 0.01] = F(1e-6)           # at the observed threshold: not observed
        return d, o, w

    gd, go, gw = layer(len(gbi))
    td, to, tw = layer(len(tbi))
    # the test layer is the gt plus noise where both exist, so the errors are small and the sum spans binades
    gslot = {tuple(b): i for i, b in enumerate(gbi.tolist())}
    for i, b in enumerate(tbi.tolist()):
        if tuple(b) in gslot:
            j = gslot[tuple(b)]
            td[i] = (gd[j] + rng.normal(0, 10.0 ** rng.uniform(-6, -1), nv)).astype(F)
    return (gbi.astype(np.int32), gd, go, gw), (tbi.astype(np.int32), td, to, tw)


def _upload(ctx, sid, vs, vps, L):
    bi, d, o, w = L
    # one array pair serves both layers: TSDF (d, w) and ESDF (d, o)
    return capi.Submap(ctx, sid, vs, vps, bi, d, w, d, o)


def _ref(gL, tL, layer, mode, vps):
    if layer == capi.EVAL_LAYER_ESDF:
        g, t = R.esdf_layer(gL[0], gL[1], gL[2]), R.esdf_layer(tL[0], tL[1], tL[2])
    else:
        g, t = R.tsdf_layer(gL[0], gL[1], gL[3]), R.tsdf_layer(tL[0], tL[1], tL[3])
    return R.evaluate_layers_rmse(g, t, mode, vps)


def _assert_details_equal(got, want):
    for k in KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("total_squared_error", "rmse", "max_error", "min_error", "min_abs_error"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])


@pytest.mark.parametrize("vps", [8, 16])
def test_evaluation_bit_exact_in_every_layer_and_mode(ctx, vps):
    rng = np.random.default_rng(vps)
    gL, tL = _esdf_pair(rng, vps, 40, 7, 9)
    g, t = _upload(ctx, 0, 0.1, vps, gL), _upload(ctx, 1, 0.1, vps, tL)
    for layer in (capi.EVAL_LAYER_ESDF, capi.EVAL_LAYER_TSDF):
        for mode in range(4):
            want, (wbi, wd, ws) = _ref(gL, tL, layer, mode, vps)
            got, (bi, d, s) = capi.evaluate_layers_rmse(g, t, layer, mode, error_layer=True)
            _assert_details_equal(got, want)
            assert got["num_evaluated_voxels"] > 1000 and (got["num_ignored_voxels"] > 1000) == (mode != 0)
            assert np.array_equal(bi, wbi) and np.array_equal(_bits(d), _bits(wd)) and np.array_equal(s, ws)
            assert capi.evaluate_layers_rmse(g, t, layer, mode) == got     # without the error layer: the same details
    g.destroy()
    t.destroy()


def test_evaluation_block_orders_and_overlap(ctx):
    """the same block sets in other slot orders give the same counts and extrema (the sum's association follows the slot
    order, so it is compared with the restatement in each order); disjoint sets evaluate nothing"""
    vps = 16
    rng = np.random.default_rng(11)
    gL, tL = _esdf_pair(rng, vps, 25, 5, 5, shuffle=False)
    base = None
    for trial in range(3):
        pg, pt = rng.permutation(len(gL[0])), rng.permutation(len(tL[0]))
        gP, tP = tuple(a[pg] for a in gL), tuple(a[pt] for a in tL)
        g, t = _upload(ctx, 0, 0.1, vps, gP), _upload(ctx, 1, 0.1, vps, tP)
        want, (wbi, wd, ws) = _ref(gP, tP, capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_TEST, vps)
        got, (bi, d, s) = capi.evaluate_layers_rmse(g, t, capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_TEST, True)
        _assert_details_equal(got, want)
        assert np.array_equal(bi, wbi) and np.array_equal(_bits(d), _bits(wd)) and np.array_equal(s, ws)
        key = tuple(got[k] for k in KEYS) + (got["max_error"], got["min_abs_error"])
        assert base is None or key == base
        base = key
        g.destroy()
        t.destroy()
    # disjoint block sets
    gL, tL = _esdf_pair(rng, 8, 0, 6, 4)
    g, t = _upload(ctx, 0, 0.1, 8, gL), _upload(ctx, 1, 0.1, 8, tL)
    got, (bi, _, _) = capi.evaluate_layers_rmse(g, t, capi.EVAL_LAYER_ESDF, capi.EVAL_ALL_VOXELS, True)
    assert got["num_non_overlapping_voxels"] == 10 * 512 and got["num_evaluated_voxels"] == 0 and got["rmse"] == 0.0
    assert len(bi) == 0
    g.destroy()
    t.destroy()


def test_identity_and_run_to_run(ctx):
    vps = 16
    rng = np.random.default_rng(5)
    gL, tL = _esdf_pair(rng, vps, 30, 4, 6)
    g, t = _upload(ctx, 0, 0.1, vps, gL), _upload(ctx, 1, 0.1, vps, tL)
    same = capi.evaluate_layers_rmse(g, g, capi.EVAL_LAYER_ESDF, capi.EVAL_ALL_VOXELS)
    obs = int(gL[2].astype(bool).sum())
    assert same["rmse"] == 0.0 and same["total_squared_error"] == 0.0 and same["max_error"] == 0.0
    assert same["num_evaluated_voxels"] == obs and same["num_non_overlapping_voxels"] == gL[2].size - obs
    runs = [capi.evaluate_layers_rmse(g, t, capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_ALL, True) for _ in range(2)]
    (d0, e0), (d1, e1) = runs
    assert d0 == d1 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(e0, e1))
    g.destroy()
    t.destroy()


def test_evaluation_errors(ctx):
    rng = np.random.default_rng(9)
    gL, tL = _esdf_pair(rng, 8, 4, 1, 1)
    g = _upload(ctx, 0, 0.1, 8, gL)
    other_vs = _upload(ctx, 1, 0.2, 8, tL)
    g16L, _ = _esdf_pair(rng, 16, 3, 0, 0)
    other_vps = _upload(ctx, 2, 0.1, 16, g16L)
    tsdf_only = capi.Submap(ctx, 3, 0.1, 8, tL[0], tL[1], tL[3])
    released = _upload(ctx, 4, 0.1, 8, tL)
    released.release_raw_layers()
    det = capi.EvaluationDetails()
    lib = ctx.lib

    def code(a, b, layer=0, mode=0, d=det):
        return lib.vgx_evaluate_layers_rmse(a.h, b.h, layer, mode, C.byref(d) if d is not None else None, None, None,
                                            None, None)

    assert code(g, other_vs) == capi.ERR_INVALID
    assert code(g, other_vps) == capi.ERR_INVALID
    assert code(g, tsdf_only, capi.EVAL_LAYER_ESDF) == capi.ERR_INVALID
    assert code(g, tsdf_only, capi.EVAL_LAYER_TSDF) == capi.OK
    assert code(g, released, capi.EVAL_LAYER_TSDF) == capi.ERR_INVALID
    assert code(g, g, 2) == capi.ERR_INVALID and code(g, g, 0, 4) == capi.ERR_INVALID and code(g, g, 0, -1) == capi.ERR_INVALID
    assert code(g, g, 0, 0, None) == capi.ERR_INVALID
    for h in (g, other_vs, other_vps, tsdf_only, released):
        h.destroy()


def _random_tsdf(rng, vps, vs, block_min, block_dims, zero_frac=0.05):
    bi = synth.dense_block_index(block_min, block_dims)
    n, nv = len(bi), vps ** 3
    d = rng.uniform(-0.3, 0.3, (n, nv)).astype(F)
    w = rng.uniform(0.5, 30, (n, nv)).astype(F)
    w[rng.random(w.shape) < zero_frac] = 0
    return type("Sm", (), dict(voxel_size=float(F(vs)), vps=vps, block_index=np.ascontiguousarray(bi, np.int32),
                               tsdf_distance=d, tsdf_weight=w))


def _layer_dict(layer):
    bi, d, w, rgba = layer.download()
    return {tuple(int(v) for v in b): (dd, ww) for b, dd, ww in zip(bi, d, w)}, rgba


def _assert_layers_equal(got, want):
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    for k in want:
        assert np.array_equal(_bits(got[k][0]), _bits(want[k][0])), k
        assert np.array_equal(_bits(got[k][1]), _bits(want[k][1])), k


@pytest.mark.parametrize("vps", [8, 16])
def test_transform_bit_exact_on_random_layers(ctx, vps):
    rng = np.random.default_rng(30 + vps)
    vs = 0.1 if vps == 16 else 0.2
    sm = _random_tsdf(rng, vps, vs, (-2, -1, -1), (4, 3, 2))
    h = capi.Submap(ctx, 0, vs, vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight)
    q = np.array([0.98, 0.1, -0.12, 0.1]) / np.linalg.norm([0.98, 0.1, -0.12, 0.1])
    for T in (_yaw_pose(0.4, (0.3, -0.2, 0.1)), np.array([1, 0, 0, 0, 0, 0, 0], F),
              np.array([*q, 0.5, 0.25, -0.3], F)):
        layer = capi.TsdfLayer(ctx, vs, vps)
        nb = layer.transform_submap(h, T)
        got, rgba = _layer_dict(layer)
        want = R.transform_layer(sm, T)
        assert nb == len(want) > 10
        _assert_layers_equal(got, want)
        assert not rgba.any()
        layer.destroy()
    h.destroy()


def test_transform_city_scene(ctx):
    vs, vps = 0.1, 16
    p = np.array([0.3, -0.2, 0.05, 0.2])
    sm = capi.Submap.synth_city(ctx, 0, vs, vps, (-4, -4, -4), (8, 8, 8), 0.3, 2.0, 10.0, p, 3)
    td, tw, _, _ = sm.download_layers(vps)
    ref = type("Sm", (), dict(voxel_size=float(F(vs)), vps=vps, block_index=sm.block_index(), tsdf_distance=td,
                              tsdf_weight=tw))
    T = _yaw_pose(-0.07, (0.13, 0.04, -0.02))
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.transform_submap(sm, T)
    _assert_layers_equal(_layer_dict(layer)[0], R.transform_layer(ref, T))
    layer.destroy()
    sm.destroy()


def test_transform_errors_leave_the_layer_untouched(ctx):
    rng = np.random.default_rng(8)
    s16 = _random_tsdf(rng, 16, 0.1, (-1, -1, -1), (2, 2, 2))
    s8 = _random_tsdf(rng, 8, 0.1, (-1, -1, -1), (2, 2, 2))
    s_vs = _random_tsdf(rng, 16, 0.2, (-1, -1, -1), (2, 2, 2))
    up = [capi.Submap(ctx, i, s.voxel_size, s.vps, s.block_index, s.tsdf_distance, s.tsdf_weight)
          for i, s in enumerate((s16, s8, s_vs, s16))]
    ok, wrong_vps, wrong_vs, released = up
    released.release_raw_layers()
    ident = np.array([1, 0, 0, 0, 0, 0, 0], F)
    empty = capi.TsdfLayer(ctx, 0.1, 16)
    full = capi.TsdfLayer(ctx, 0.1, 16)
    full.upload(synth.dense_block_index((0, 0, 0), (2, 1, 1)), rng.uniform(-1, 1, (2, 4096)).astype(F),
                rng.uniform(0, 1, (2, 4096)).astype(F))
    before_full = full.download()

    def refused(layer, sm, T, before):
        with pytest.raises(capi.VgxError) as e:
            layer.transform_submap(sm, T)
        assert e.value.code == capi.ERR_INVALID, e.value
        assert all(np.array_equal(a, b) for a, b in zip(before, layer.download()))
        return str(e.value)

    assert "not empty" in refused(full, ok, ident, before_full)
    before_empty = empty.download()
    assert "voxels_per_side" in refused(empty, wrong_vps, ident, before_empty)
    assert "voxel_size" in refused(empty, wrong_vs, ident, before_empty)
    assert "released" in refused(empty, released, ident, before_empty)
    for bad in (np.nan, np.inf):
        T = ident.copy()
        T[4] = bad
        assert "finite" in refused(empty, ok, T, before_empty)
    assert "unit" in refused(empty, ok, np.array([1.01, 0, 0, 0, 0, 0, 0], F), before_empty)
    nb = C.c_int64()
    assert ctx.lib.vgx_tsdf_layer_transform_submap(empty.h, None, None, C.byref(nb)) == capi.ERR_INVALID
    assert empty.stats()[0] == 0
    for h in up + [empty, full]:
        h.destroy()


# ---- MapEvaluation::evaluate end to end -------------------------------------------------------------------------

def _compose4(off, p):
    """T_off * T_p for 4-DoF poses (x, y, z, yaw)"""
    c, s = np.cos(off[3]), np.sin(off[3])
    return np.array([off[0] + c * p[0] - s * p[1], off[1] + s * p[0] + c * p[1], off[2] + p[2], off[3] + p[3]])


def _pose7(p):
    return _yaw_pose(p[3], p[:3])


def _city(ctx, n=4):
    vs, vps = 0.1, 16
    poses = [np.array([1.6 * k, 0.3 * np.sin(k), 0.03 * k, 0.1 * k]) for k in range(n)]
    subs = [capi.Submap.synth_city(ctx, k, vs, vps, (-4, -4, -4), (8, 8, 8), 0.3, 2.0, 10.0, p, 3)
            for k, p in enumerate(poses)]
    return vs, vps, poses, subs


def _ground_truth(ctx, subs, poses4, vs, vps, sid=100):
    layer = capi.TsdfLayer(ctx, vs, vps)
    capi.projected_map(ctx, subs, np.stack([_pose7(p) for p in poses4]), layer)
    gt = capi.Submap.from_tsdf_layer(ctx, layer, sid)
    layer.destroy()
    return gt


class _Align:
    """alignSubmapAtoSubmapB: the reference constant at 0, the reading's 4-DoF pose solved from 0 by the harness LM over
    one kVoxels RegistrationCostFunction(reference, reading) (ESDF distance, every point)"""

    def __init__(self, ctx):
        self.ctx, self.summary = ctx, None

    def __call__(self, reference, reading):
        from harness import lm
        from harness.backends import GpuBackend
        cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=-1.0, use_esdf_distance=1)
        cf = capi.RegistrationCostFunction(self.ctx, reference, reading, cfg)
        batch = capi.RegistrationBatch(self.ctx, [cf], [(0, 1)])
        x, self.summary = lm.solve(lm.Problem(GpuBackend(capi, self.ctx, batch, 2), 2, [(0, 1)]), np.zeros((2, 4)),
                                   parameter_tolerance=1e-12, max_iterations=200, max_seconds=120)
        batch.destroy()
        cf.destroy()
        return x[1]


def test_map_evaluation_identical_maps(ctx):
    """A ground truth equal to the projected map: the alignment stays at exactly 0, the transform is then a copy of every
    voxel that interpolates (TSDF rmse exactly 0), and the ESDF rmse is what the regeneration leaves: the transform does
    not write a voxel whose +x/+y/+z neighbours are unobserved (section 10's rule), so the regenerated ESDF differs near
    those voxels by at most a voxel."""
    vs, vps, poses, subs = _city(ctx)
    gt = _ground_truth(ctx, subs, poses, vs, vps)
    align = _Align(ctx)
    T7 = np.stack([_pose7(p) for p in poses])
    out = capi.map_evaluation(ctx, subs, T7, gt, align)
    det = out["details"]
    assert np.array_equal(out["pose4"], np.zeros(4)), out["pose4"]
    assert np.array_equal(out["T_ground_truth__reading"], [1, 0, 0, 0, 0, 0, 0])
    assert det["num_evaluated_voxels"] > 100000 and det["rmse"] < 0.1 * vs and det["max_error"] <= vs * 1.0001, det
    # the identity transform on its own: TSDF layers equal wherever the copy wrote, with exact counts
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.transform_submap(gt, np.array([1, 0, 0, 0, 0, 0, 0], F))
    gt_t = capi.Submap.from_tsdf_layer(ctx, layer, 101)
    written = int((layer.download()[2] > F(1e-6)).sum())
    for mode in range(4):
        same = capi.evaluate_layers_rmse(gt_t, gt, capi.EVAL_LAYER_TSDF, mode)
        assert same["rmse"] == 0.0 and same["total_squared_error"] == 0.0 and same["max_error"] == 0.0, same
        assert same["num_overlapping_voxels"] == written > 100000
    layer.destroy()
    for h in subs + [gt, gt_t]:
        h.destroy()


def test_map_evaluation_recovers_an_offset_ground_truth(ctx):
    vs, vps, poses, subs = _city(ctx)
    off = np.array([0.06, -0.04, 0.02, np.deg2rad(1.5)])
    gt = _ground_truth(ctx, subs, [_compose4(off, p) for p in poses], vs, vps)
    align = _Align(ctx)
    out = capi.map_evaluation(ctx, subs, np.stack([_pose7(p) for p in poses]), gt, align)
    T = out["T_ground_truth__reading"]
    yaw = 2 * np.arctan2(T[3], T[0])
    print("alignment", out["pose4"], align.summary["iterations"], align.summary["termination"], out["details"])
    assert np.abs(T[4:7] - off[:3]).max() < 1e-3 and abs(np.rad2deg(yaw - off[3])) < 0.01, (T, off)
    assert abs(T[1]) < 1e-12 and abs(T[2]) < 1e-12
    det = out["details"]
    assert det["num_evaluated_voxels"] > 100000 and det["rmse"] < 0.02, det
    for h in subs + [gt]:
        h.destroy()
