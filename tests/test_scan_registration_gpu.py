"""Scan-to-map registration on the device (vgx_scan_registration) against the restatement of
tests/scan_registration_ref.py, bit for bit: `evaluate` on a random uploaded layer (holes, shuffled slots, zero weights,
vps 8 and 16; points inside, outside, on faces, non-finite; every size at which the partition takes another path; stride,
range limits; host, device and vgx_scan sources), on the layer the reproducible integrator built (one that grew its block
table included), `refine` on the six seeded priors and on every usable = 0 path, the stream ordering behind an
asynchronous scan, and every refusal."""
import math

import numpy as np
import pytest

from tests import scan_registration_ref as R
from tests.test_map_query_gpu import _full_pose, _points, _random_submap, _yaw_pose
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
# n = 0, one point, around a wave, around one trip of a workgroup's threads (255 .. 257: the second trip starts at 257),
# around one workgroup's quota (1023 .. 1025: the second partial), and where the partials pass the fold's 256 threads
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1]
DELTA = (0.03, -0.02, 0.01, 0.02)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want):
    """(out, n_valid, n_candidates) of the library and of the restatement"""
    assert (got[1], got[2]) == (want[1], want[2]), (got[1:], want[1:])
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])


def _sensor_points(rng, d, n, T):
    """layer-frame points of every kind seen from the sensor frame of pose T, with non-finite ones strewn in"""
    p = _points(rng, d, n)
    p = p[rng.permutation(len(p))]
    q = np.array([T[0], -T[1], -T[2], -T[3]], F)
    pc = R.quat_rotate(q, (p - T[4:]).astype(F))
    bad = rng.random(len(pc)) < 0.02
    pc[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf, 3e38], int(bad.sum())).astype(F)
    return np.ascontiguousarray(pc, F)


@pytest.fixture(scope="module", params=[8, 16])
def random_scene(request, ctx):
    vps = request.param
    rng = np.random.default_rng(40 + vps)
    d = _random_submap(rng, vps)
    layer = capi.TsdfLayer(ctx, d.voxel_size, vps)
    layer.upload(d.block_index, d.tsdf_distance, d.tsdf_weight)
    L = R.layer_of(d.voxel_size, vps, d.block_index, d.tsdf_distance, d.tsdf_weight)
    T = _full_pose(rng) if vps == 8 else _yaw_pose(0.7, (0.3, -0.2, 0.1))
    pc = _sensor_points(rng, d, 150000, T)
    assert len(pc) > max(SIZES)
    yield layer, L, T, pc
    layer.destroy()


def test_evaluate_on_a_random_layer_at_every_size(ctx, random_scene):
    layer, L, T, pc = random_scene
    cfg = dict(max_abs_distance_m=0.25)
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(**cfg))
    for n in SIZES:
        reg.set_points(pc[:n])
        got = reg.evaluate(layer, T, DELTA)
        _same(got, R.evaluate(L, pc[:n], T, DELTA, R.config(**cfg)))
        if n > 1000:
            assert 0 < got[1] < got[2] < n                   # invalid neighbours, distances and non-finite points all cut
    # the number of candidates, not of points, decides the partition: stride 3 at the same thresholds
    cfg3 = dict(max_abs_distance_m=0.25, point_stride=3)
    reg3 = capi.ScanRegistration(ctx, capi.scan_registration_config(**cfg3))
    for n in (1, 2, 3, 4, 3 * 256, 3 * 256 + 1, 3 * 1024, 3 * 1024 + 1, 3 * 1024 + 4, 100000):
        reg3.set_points(pc[:n])
        _same(reg3.evaluate(layer, T, DELTA), R.evaluate(L, pc[:n], T, DELTA, R.config(**cfg3)))
    reg.destroy()
    reg3.destroy()


def test_evaluate_with_range_limits_and_corrections(ctx, random_scene):
    layer, L, T, pc = random_scene
    n = 20000
    r = np.sqrt((pc[:n].astype(np.float64) ** 2).sum(1))
    lo, hi = np.nanpercentile(np.where(np.isfinite(r), r, np.nan), [25, 75])
    for cfg in (dict(max_abs_distance_m=0.25, min_range_m=float(lo), max_range_m=float(hi)),
                dict(max_abs_distance_m=0.1, min_range_m=float(lo), point_stride=3),
                dict(max_abs_distance_m=1e9, max_range_m=float(hi))):
        reg = capi.ScanRegistration(ctx, capi.scan_registration_config(**cfg))
        reg.set_points(pc[:n])
        for delta in ((0.0, 0.0, 0.0, 0.0), DELTA, (-0.4, 0.3, 0.2, -1.3), (0.0, 0.0, 0.0, math.pi)):
            got = reg.evaluate(layer, T, delta)
            _same(got, R.evaluate(L, pc[:n], T, delta, R.config(**cfg)))
            assert 0 < got[1] <= got[2] < n // cfg.get("point_stride", 1)
        reg.destroy()


def test_host_device_and_scan_sources_agree(ctx, random_scene):
    import torch
    layer, L, T, pc = random_scene
    pts = pc[:5000][np.isfinite(pc[:5000]).all(1)]              # (a decoded scan holds finite points only)
    cfg = dict(max_abs_distance_m=0.25, point_stride=2)
    want = R.evaluate(L, pts, T, DELTA, R.config(**cfg))
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(**cfg))
    reg.set_points(pts)
    _same(reg.evaluate(layer, T, DELTA), want)
    dev = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    reg.set_points(dev)
    _same(reg.evaluate(layer, T, DELTA), want)
    reg.set_points(dev.data_ptr(), len(pts))
    _same(reg.evaluate(layer, T, DELTA), want)
    scan = capi.Scan(ctx)
    msg = pc[:5000].copy()                                       # the raw message: the decode drops the non-finite points
    layout = capi.scan_layout(width=len(msg), height=1, point_step=12, offset_x=0, offset_y=4, offset_z=8,
                              color_kind=capi.SCAN_COLOR_NONE)
    assert scan.decode_msg(layout, msg.tobytes())[0] == len(pts)
    reg.set_points(scan)
    _same(reg.evaluate(layer, T, DELTA), want)
    assert scan.decode_msg(capi.scan_layout(width=1000, height=1, point_step=12, offset_x=0, offset_y=4, offset_z=8,
                                            color_kind=capi.SCAN_COLOR_NONE), pts[:1000].tobytes())[0] == 1000
    _same(reg.evaluate(layer, T, DELTA), R.evaluate(L, pts[:1000], T, DELTA, R.config(**cfg)))   # borrowed: the scan as it stands
    reg.destroy()
    scan.destroy()


def _integrated_layer(ctx, n_scans=6, **layer_kw):
    layer = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS, **layer_kw)
    integrator = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for k in range(n_scans):
        integrator.integratePointCloud(R.pose7(R.scan_pose(k)), R.room_scan(R.scan_pose(k)))
    return layer, integrator


@pytest.fixture(scope="module")
def room(ctx):
    layer, integrator = _integrated_layer(ctx)
    yield layer, R.room_layer(), R.room_scan(R.scan_pose(6))
    integrator.destroy()
    layer.destroy()


def test_evaluate_on_the_integrated_layer(ctx, room):
    """the reproducible integrator's layer against the restatement on the CPU oracle's layer"""
    layer, L, pts = room
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE))
    reg.set_points(pts)
    for seed in range(6):
        T = R.pose7(R.seeded_prior(seed))
        got = reg.evaluate(layer, T)
        _same(got, R.evaluate(L, pts, T, [0.0] * 4, R.config(R.MAX_ABS_DISTANCE)))
        assert got[1] >= 0.5 * got[2] and got[2] == len(pts)
    # a layer that started with a one-block table and pool and grew both while the scans came in
    grown, integrator = _integrated_layer(ctx, lut_min=(0, 0, 0), lut_dim=(1, 1, 1), max_blocks=1)
    assert grown.growths() > 0
    T = R.pose7(R.seeded_prior(1))
    _same(reg.evaluate(grown, T, DELTA), R.evaluate(L, pts, T, DELTA, R.config(R.MAX_ABS_DISTANCE)))
    integrator.destroy()
    grown.destroy()
    reg.destroy()


def _same_refinement(reg, got, want):
    T, usable, delta, S = got
    wT, wdelta, wS, whistory = want
    assert np.array_equal(_bits(T), _bits(wT)) and usable == bool(wS["usable"])
    assert np.array_equal(_bits(delta), _bits(wdelta)), (delta, wdelta)
    for key in ("usable", "termination", "num_iterations", "num_successful_steps", "num_evaluations", "num_factorization_failures",
                "n_candidates", "n_valid_first", "n_valid_last"):
        assert S[key] == wS[key], (key, S[key], wS[key])
    for key in ("initial_cost", "final_cost"):
        assert np.array_equal(_bits(np.float64(S[key])), _bits(np.float64(wS[key]))), key
    history = reg.history()
    assert len(history) == len(whistory)
    for k, (h, wh) in enumerate(zip(history, whistory)):
        for key in ("cost", "trial_cost", "gain_ratio", "radius", "step_norm"):
            assert np.array_equal(_bits(np.float64(h[key])), _bits(np.float64(wh[key]))), (k, key, h[key], wh[key])
        assert (h["accepted"], h["factorization_failed"]) == (wh["accepted"], wh["factorization_failed"])


def test_refine_on_the_seeded_priors(ctx, room):
    layer, L, pts = room
    cfg = R.config(R.MAX_ABS_DISTANCE)
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE))
    reg.set_points(pts)
    truth = R.scan_pose(6)
    for seed in range(6):
        prior = R.pose7(R.seeded_prior(seed))
        got = reg.refine(layer, prior)
        _same_refinement(reg, got, R.refine(L, pts, prior, cfg))
        assert got[1] and got[3]["termination_type"] == capi.CONVERGENCE
        assert R.pose_error(got[0], truth)[0] < R.pose_error(prior, truth)[0] or seed == 0   # (seed 0 starts 3 cm off)
    reg.destroy()


def test_unusable_refinements_return_the_prior(ctx, room):
    layer, L, pts = room
    cfg = R.config(R.MAX_ABS_DISTANCE)
    prior = R.pose7(R.seeded_prior(2))
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE))
    # no convergence within one iteration: delta is what the solve ended at, the pose is the prior's bits
    reg.set_points(pts)
    got = reg.refine(layer, prior, max_num_iterations=1)
    _same_refinement(reg, got, R.refine(L, pts, prior, cfg, max_num_iterations=1))
    assert not got[1] and got[3]["termination_type"] == capi.NO_CONVERGENCE and got[2].any()
    assert np.array_equal(_bits(got[0]), _bits(prior))
    # an empty layer; a scan without a finite point; no point at all; a ratio nobody reaches
    empty = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS)
    Lempty = R.layer_of(R.VOXEL_SIZE, R.VPS, np.zeros((0, 3), np.int32), np.zeros((0, R.VPS ** 3), F), np.zeros((0, R.VPS ** 3), F))
    invalid = np.full((500, 3), np.nan, F)
    invalid[::3] = np.inf
    for lay, Lr, points in ((empty, Lempty, pts), (layer, L, invalid), (layer, L, pts[:0])):
        reg.set_points(points)
        got = reg.refine(lay, prior)
        _same_refinement(reg, got, R.refine(Lr, points, prior, cfg))
        assert not got[1] and got[3]["num_iterations"] == 0 and got[3]["termination_type"] == capi.FAILURE
        assert got[3]["termination_reason"] == capi.TERMINATION_TOO_FEW_POINTS and not got[2].any()
        assert np.array_equal(_bits(got[0]), _bits(prior))
    strict = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE, min_valid_ratio=0.99))
    strict.set_points(pts)
    got = strict.refine(layer, prior)
    _same_refinement(strict, got, R.refine(L, pts, prior, R.config(R.MAX_ABS_DISTANCE, min_valid_ratio=0.99)))
    assert not got[1] and got[3]["num_iterations"] == 0
    for x in (strict, reg, empty):
        x.destroy()


def test_refine_is_ordered_behind_an_asynchronous_scan(ctx, room):
    """a refine issued right after vgx_tsdf_integrate(n_updates = NULL) sees that scan: the bits of the same call after
    vgx_ctx_synchronize_tsdf, which are the restatement's on the six-scan layer"""
    _, L, pts = room
    prior = R.pose7(R.seeded_prior(4))
    results = []
    for wait in (False, True):
        layer, integrator = _integrated_layer(ctx, n_scans=5)
        reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE))
        reg.set_points(pts)
        integrator.integratePointCloud(R.pose7(R.scan_pose(5)), R.room_scan(R.scan_pose(5)), count=False)
        if wait:
            ctx.synchronize_tsdf()
        got = reg.refine(layer, prior)
        results.append((got, reg.history()))
        _same_refinement(reg, got, R.refine(L, pts, prior, R.config(R.MAX_ABS_DISTANCE)))
        for x in (reg, integrator, layer):
            x.destroy()
    (a, ha), (b, hb) = results
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2])) and ha == hb


def test_refusals(ctx, room):
    layer, _, pts = room
    lib = ctx.lib
    good = capi.scan_registration_config(R.MAX_ABS_DISTANCE)
    prior = R.pose7(R.seeded_prior(0))

    def refused(fn, code=capi.ERR_INVALID):
        with pytest.raises(capi.VgxError) as e:
            fn()
        assert e.value.code == code, e.value

    # the configuration, at creation: no default distance; stride; ranges; NULL
    for kw in (dict(max_abs_distance_m=0.0), dict(max_abs_distance_m=-1.0), dict(max_abs_distance_m=math.inf),
               dict(max_abs_distance_m=math.nan), dict(max_abs_distance_m=0.5, point_stride=0),
               dict(max_abs_distance_m=0.5, min_range_m=2.0, max_range_m=1.0), dict(max_abs_distance_m=0.5, min_range_m=math.nan),
               dict(max_abs_distance_m=0.5, min_valid_ratio=math.nan)):
        refused(lambda: capi.ScanRegistration(ctx, capi.scan_registration_config(**kw)))
    refused(lambda: capi.ScanRegistration(ctx, None))
    h = capi.vp()
    assert lib.vgx_scan_registration_create(ctx.h, capi.C.byref(good), None) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_create(None, capi.C.byref(good), capi.C.byref(h)) == capi.ERR_INVALID
    for fn in (lib.vgx_scan_registration_destroy,):
        assert fn(None) == capi.ERR_INVALID

    reg = capi.ScanRegistration(ctx, good)
    refused(lambda: reg.evaluate(layer, prior))                              # no points set
    refused(lambda: reg.refine(layer, prior))
    assert lib.vgx_scan_registration_set_points(reg.h, None, 5) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_points(reg.h, None, -1) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_points_device(reg.h, None, 5) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_scan(reg.h, None) == capi.ERR_INVALID
    refused(lambda: reg.evaluate(layer, prior))                              # ... still none
    reg.set_points(pts)
    out, T, delta = np.full(15, 7.0), capi._f32(prior), np.zeros(4)
    nv, nc = capi.C.c_int64(-1), capi.C.c_int64(-1)
    f32p, f64p = capi.f32p, capi.f64p

    def evaluate(layer_h=layer.h, T=T, delta=delta, out=out):
        return lib.vgx_scan_registration_evaluate(reg.h, layer_h, capi._ptr(T, f32p), capi._ptr(delta, f64p), capi._ptr(out, f64p),
                                                  capi.C.byref(nv), capi.C.byref(nc))

    Tr, dr = np.full(7, 7.0, F), np.full(4, 7.0)

    def refine(layer_h=layer.h, T=T, Tr=Tr, dr=dr):
        return lib.vgx_scan_registration_refine(reg.h, layer_h, capi._ptr(T, f32p), None, capi._ptr(Tr, f32p), capi._ptr(dr, f64p), None)

    nan_T, inf_T, long_T = T.copy(), T.copy(), T.copy()
    nan_T[5], inf_T[0] = np.nan, np.inf
    long_T[:4] *= F(1.0001)
    other = capi.Context(0)
    foreign = capi.TsdfLayer(other, R.VOXEL_SIZE, R.VPS)
    foreign_scan = capi.Scan(other)
    for rc in (evaluate(layer_h=None), evaluate(T=None), evaluate(delta=None), evaluate(out=None), evaluate(T=nan_T), evaluate(T=inf_T),
               evaluate(T=long_T), evaluate(delta=np.array([0, np.nan, 0, 0.0])), evaluate(delta=np.array([0, 0, 0, np.inf])),
               evaluate(layer_h=foreign.h), refine(layer_h=None), refine(T=None), refine(Tr=None), refine(dr=None), refine(T=nan_T),
               refine(T=long_T), refine(layer_h=foreign.h), lib.vgx_scan_registration_set_scan(reg.h, foreign_scan.h),
               lib.vgx_scan_registration_evaluate(None, layer.h, capi._ptr(T, f32p), capi._ptr(delta, f64p), capi._ptr(out, f64p), None, None),
               lib.vgx_scan_registration_history(reg.h, -1, None, None), lib.vgx_scan_registration_history(reg.h, 2, None, None)):
        assert rc == capi.ERR_INVALID
    assert "another context" in lib.vgx_last_error(ctx.h).decode() or "history" in lib.vgx_last_error(ctx.h).decode()
    # nothing was written by any refused call
    assert (out == 7.0).all() and (Tr == 7.0).all() and (dr == 7.0).all() and (nv.value, nc.value) == (-1, -1)
    assert evaluate() == capi.OK and nc.value == len(pts) and (out != 7.0).all()     # (the points set before are still set)
    # too many candidates for one launch: refused before anything is read
    reg.set_points(1 << 20, (2 ** 31 - 1) * 1024 + 1)                               # (an address nobody dereferences)
    assert evaluate() == capi.ERR_UNSUPPORTED and refine() == capi.ERR_UNSUPPORTED
    # a layer of another voxels_per_side cannot be made (vgx_tsdf_layer_create refuses it), so that refusal is unreachable
    refused(lambda: capi.TsdfLayer(ctx, 0.1, 4), capi.ERR_UNSUPPORTED)
    for x in (reg, foreign, foreign_scan):
        x.destroy()
    other.close()


def test_special_voxel_values_fall_under_the_stated_comparisons(ctx):
    """One point in the cube CELL of tests/special_voxel_scene.py's layer (D = Z0 - z, r = 0.0275 there), identity prior,
    no correction; a special value planted into CELL.  The expectations are IEEE's under the header's comparisons --
    "every weight is > 0", "|D| < max_abs_distance_m" -- written down by hand."""
    from tests import special_voxel_scene as Z
    bi, d, w = Z.layer()
    layer = capi.TsdfLayer(ctx, Z.VOXEL_SIZE, Z.VPS)
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(0.2))
    reg.set_points(np.array([[Z.X, Z.Y, Z.Z_IN]], F))
    identity = np.array([1, 0, 0, 0, 0, 0, 0], F)

    def evaluate(dd=d, ww=w):
        layer.upload(bi, dd, ww)
        return reg.evaluate(layer, identity)

    def no_term(got):
        return got[1:] == (0, 1) and not _bits(got[0]).any()                      # a candidate, not usable; every sum +0

    nb7, cell, other = [Z.NEIGHBOUR_7], Z.CELL, [Z.CELL[1]]
    base = evaluate()
    assert base[1:] == (1, 1) and abs(base[0][0] - 0.0275 ** 2) < 1e-6 and abs(base[0][3] + 0.0275) < 1e-4      # sum r r, sum J_z r
    # weight 1e-40 (a denormal) and +inf are > 0: the voxel is observed, the point usable, the sums those of weight 1
    for value in Z.WEIGHTS_OBSERVED:
        got = evaluate(ww=Z.plant(bi, w, nb7, value))
        assert got[1:] == (1, 1) and np.array_equal(_bits(got[0]), _bits(base[0])), value
    # weight NaN, -0.0, 0.0, -1 are not > 0: not observed, the point not usable
    for value in Z.WEIGHTS_UNOBSERVED:
        assert no_term(evaluate(ww=Z.plant(bi, w, nb7, value))), value
    # distance NaN, +inf, -inf (in neighbour 7 they reach r as they are; in another the inf meets its negation: NaN) and
    # 3e38: |r| < max_abs_distance_m fails for an infinity, for a NaN and for 1e37: no term
    for where, value in ((nb7, np.nan), (nb7, np.inf), (nb7, -np.inf), (other, np.inf), (other, -np.inf), (nb7, 3e38), (cell, 3e38)):
        assert no_term(evaluate(Z.plant(bi, d, where, value))), value
    # -0.0, 0.0 and 1e-40 in one neighbour are ordinary values: the same bits from all three, not the unplanted ones
    sums = [evaluate(Z.plant(bi, d, nb7, value)) for value in (-0.0, 0.0, 1e-40)]
    assert all(g[1:] == (1, 1) for g in sums) and len({g[0].tobytes() for g in sums}) == 1 and sums[0][0][0] != base[0][0]
    # all 8 neighbours -0.0: r is a zero, |r| < max: usable, every term a zero
    got = evaluate(Z.plant(bi, d, cell, -0.0))
    assert got[1:] == (1, 1) and not got[0].any()
    # all 8 neighbours 1e-40: r = 1e-40 exactly (every coefficient but c0 is x - x = 0), a residual like any other: its
    # square, exact in f64, is the sum -- a device that flushed denormals would give 0
    got = evaluate(Z.plant(bi, d, cell, 1e-40))
    assert got[1:] == (1, 1) and got[0][0] == float(F(1e-40)) ** 2 > 0 and not got[0][1:].any()
    reg.destroy()
    layer.destroy()
