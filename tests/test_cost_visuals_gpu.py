"""Cost-function visuals on the GPU (vgx_reg_evaluate_visuals) against the numpy restatement (tests/cost_visuals_ref.py)
fed from the CPU oracle's rows and, where it was built, from the reference's own compiled RegistrationCostFunction.
Scenes: oracle/synth.config1_pair (and the same scene blocked by 8), points installed through vgx_submap_set_points with
weights that make factor a power of two, so the restatement recovers the unscaled values exactly; every comparison is
bit for bit unless stated."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from oracle import ref_reg
from oracle import synth
from tests import cost_visuals_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
F = np.float32
TILE = 1024  # kTilePoints: 256 threads x 4 points
REF_POSE = np.array([0.31, -0.22, 0.05, 0.04])
READ_POSE = np.array([0.36, -0.16, 0.02, -0.03])


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi
    return capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    """vps -> (submap data, its kVoxels points, an even number of them)"""
    out = {}
    sm16, _ = synth.config1_pair()
    sm8 = synth.make_submap(synth.sphere_ground_sdf((3.2, 3.2, 3.2), 2.0, 0.45), 0.10, 8, (0, 0, 0), (8, 8, 8), trunc=0.3)
    for sm in (sm16, sm8):
        xyz, dist, w = H.oracle_points(sm)
        n = len(w) & ~1
        assert n >= 4 * TILE
        out[sm.vps] = (sm, (xyz[:n], dist[:n]))
    return out


def weights(kind, n):
    if kind == "ones":
        w = np.ones(n, F)
    elif kind == "quarters":  # equal counts of 0.25 and 0.75, interleaved
        w = np.where(np.arange(n) % 2 == 0, F(0.25), F(0.75)).astype(F)
    else:  # "halves": every weight 0.5 -- factor 2 for an odd count too
        w = np.full(n, 0.5, F)
    want = 1.0 if kind == "ones" else 2.0
    assert R.factor_of(w) == want, (kind, n)  # n / sum(w) exactly a power of two, checked on the CPU
    return w, want


def gpu_eval(cf, vis, ref_pose, read_pose, want_jac=True, want_ref=True, want_read=True, cloud=True, gradients=True):
    n = cf.num_residuals()
    r = np.full(n, np.nan)
    jo = np.full((n, 4), np.nan) if (want_jac and want_ref) else None
    je = np.full((n, 4), np.nan) if (want_jac and want_read) else None
    ok = cf.evaluate_visuals([ref_pose, read_pose], r, [jo, je] if want_jac else None, vis, cloud, gradients)
    return ok, r, jo, je


def check_against(vis, xyz, rows, factor, ref_pose, read_pose, what):
    ok, r, _, je = rows
    assert ok
    cloud, arrows, origins, f = vis.download()
    want = R.visuals(xyz, r, je, factor, ref_pose, read_pose)
    assert f == factor, what
    assert R.same(cloud, want[0]), (what, "cloud")
    assert R.same(arrows, want[1]), (what, "arrows")
    assert R.same(origins, want[2]), (what, "origins")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("vps", [8, 16])
@pytest.mark.parametrize("use_esdf", [1, 0])
def test_against_the_oracle_and_the_reference_source(capi, ctx, scenes, use_esdf, vps, layout):
    sm, (xyz, dist) = scenes[vps]
    ctx.set_brick_layout(layout)
    g = H.gpu_submap(capi, ctx, sm, 30)
    ctx.set_brick_layout(0)
    layer = H.oracle_layer(sm, bool(use_esdf))
    vis = capi.RegVisuals(ctx)
    for kind in ("ones", "quarters"):
        w, factor = weights(kind, len(xyz))
        g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
        cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS,
                                                                          use_esdf_distance=use_esdf))
        ok, r, jo, je = gpu_eval(cf, vis, REF_POSE, READ_POSE)
        assert ok and vis.stats() == (len(w), len(w))
        rows = orc.reg_evaluate(layer, xyz, dist, w, REF_POSE, READ_POSE)
        assert np.count_nonzero(rows[1]) > len(w) // 2
        check_against(vis, xyz, (rows[0], rows[1], rows[2], rows[3]), factor, REF_POSE, READ_POSE, ("oracle", kind))
        if ref_reg.available():
            Rs = ref_reg.Submap(0, np.zeros(4), sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight,
                                sm.esdf_distance, sm.esdf_observed)
            Rs.set_points(ref_reg.POINTS_VOXELS, xyz, dist, w)
            rcf = ref_reg.RegistrationCostFunction(Rs, Rs, use_esdf_distance=bool(use_esdf))
            check_against(vis, xyz, rcf.Evaluate(REF_POSE, READ_POSE), factor, REF_POSE, READ_POSE, ("reference", kind))
        cf.destroy()
    vis.destroy()
    g.destroy()


@pytest.fixture(scope="module")
def pair16(capi, ctx, scenes):
    sm, (xyz, dist) = scenes[16]
    g = H.gpu_submap(capi, ctx, sm, 31)
    yield sm, g, xyz, dist
    g.destroy()


def test_same_evaluation_rows(capi, ctx, pair16):
    """the rows are vgx_reg_evaluate's, bit for bit, with every combination of Jacobian blocks"""
    sm, g, xyz, dist = pair16
    w, _ = weights("quarters", len(xyz))
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    vis = capi.RegVisuals(ctx)
    n = len(w)
    for want_jac, want_ref, want_read in ((True, True, True), (True, False, True), (True, True, False), (False, False, False)):
        r0 = np.full(n, np.nan)
        jo0 = np.full((n, 4), np.nan) if (want_jac and want_ref) else None
        je0 = np.full((n, 4), np.nan) if (want_jac and want_read) else None
        assert cf.Evaluate([REF_POSE, READ_POSE], r0, [jo0, je0] if want_jac else None)
        ok, r, jo, je = gpu_eval(cf, vis, REF_POSE, READ_POSE, want_jac, want_ref, want_read)
        assert ok and R.same(r, r0)
        assert (jo is None and jo0 is None) or R.same(jo, jo0)
        assert (je is None and je0 is None) or R.same(je, je0)
        assert vis.stats() == (n, n if want_jac else 0)
    cf.destroy()
    vis.destroy()


def test_same_evaluation_sampling(capi, ctx, pair16):
    """sampling_ratio 0.5 on a private seed: one cost function through each entry point gives the same rows call after
    call (one evaluation's engine outputs each), and the cloud shows that evaluation's draws in draw order"""
    sm, g, xyz, dist = pair16
    w = (np.random.default_rng(7).uniform(0.1, 1.0, len(xyz))).astype(F)
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=0.5, sampler_seed=1234)
    cf_a = capi.RegistrationCostFunction(ctx, g, g, cfg)
    cf_b = capi.RegistrationCostFunction(ctx, g, g, cfg)
    vis = capi.RegVisuals(ctx)
    n = cf_a.num_residuals()
    assert n == int(F(0.5) * F(len(w)))
    acc, cum = 0.0, np.zeros(len(w))
    for i, v in enumerate(w.astype(np.float64)):
        acc = v if i == 0 else acc + v
        cum[i] = acc
    eng = orc.Mt19937(1234)
    layer = H.oracle_layer(sm)
    for call in range(2):
        idx = np.array([eng.weighted_draw(cum) for _ in range(n)], np.int64)
        r0, jo0, je0 = np.zeros(n), np.zeros((n, 4)), np.zeros((n, 4))
        assert cf_a.Evaluate([REF_POSE, READ_POSE], r0, [jo0, je0])
        ok, r, jo, je = gpu_eval(cf_b, vis, REF_POSE, READ_POSE)
        assert ok and R.same(r, r0) and R.same(jo, jo0) and R.same(je, je0), call
        cloud, arrows, origins, factor = vis.download()
        assert factor == 1.0 and len(cloud) == n and len(origins) == n
        p_m = R.mission_points(xyz[idx], REF_POSE, READ_POSE)
        assert R.same(cloud.view(F).reshape(n, 8)[:, :3], p_m), call
        rows = orc.reg_evaluate(layer, xyz, dist, w, REF_POSE, READ_POSE, sample_idx=idx)
        check_against(vis, xyz[idx], rows, 1.0, REF_POSE, READ_POSE, ("sampling", call))
    cf_a.destroy()
    cf_b.destroy()
    vis.destroy()


@pytest.mark.parametrize("n", [1, TILE - 1, TILE + 1, 2 * TILE + 3])
def test_row_counts_around_the_tile(capi, ctx, pair16, n):
    """odd counts: the paired 24-byte origin stores end on a lone double, and the tail tile is partial"""
    sm, g, xyz, dist = pair16
    w, factor = weights("halves", n)
    step = len(xyz) // n
    x, d = xyz[::step][:n], dist[::step][:n]
    g.set_points(capi.POINTS_VOXELS, x, d, w)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    vis = capi.RegVisuals(ctx)
    ok, r, jo, je = gpu_eval(cf, vis, REF_POSE, READ_POSE)
    assert ok and vis.stats() == (n, n)
    check_against(vis, x, orc.reg_evaluate(H.oracle_layer(sm), x, d, w, REF_POSE, READ_POSE), factor, REF_POSE, READ_POSE, n)
    cf.destroy()
    vis.destroy()


def test_reading_submap_far_away_every_tile_cullable(capi, ctx, pair16):
    """100 m apart with no_correspondence_cost 0.25: the rows kernel may cull its tiles, the visuals may not"""
    sm, g, xyz, dist = pair16
    w, factor = weights("quarters", len(xyz))
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS,
                                                                      no_correspondence_cost=0.25))
    vis = capi.RegVisuals(ctx)
    read_pose = READ_POSE + np.array([100.0, 0, 0, 0])
    ok, r, jo, je = gpu_eval(cf, vis, REF_POSE, read_pose)
    assert ok and not je.any()
    cloud, arrows, origins, f = vis.download()
    rec = cloud.view(F).reshape(-1, 8)
    assert R.same(rec[:, :3], R.mission_points(xyz, REF_POSE, read_pose))
    want = ((w.astype(np.float64) * 0.25).astype(F).astype(np.float64) * factor).astype(F)
    assert R.same(rec[:, 4], want) and want.all()
    assert R.same(arrows[1::2], origins) and R.same(arrows[0::2], origins)
    rows = orc.reg_evaluate(H.oracle_layer(sm), xyz, dist, w, REF_POSE, read_pose, no_correspondence_cost=0.25)
    check_against(vis, xyz, rows, factor, REF_POSE, read_pose, "far")
    cf.destroy()
    # ... and with the default cost of 0 (the tiles ARE culled by the rows kernel): positions all the same, intensity 0
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    ok, r, jo, je = gpu_eval(cf, vis, REF_POSE, read_pose)
    assert ok and not r.any()
    rec = vis.download()[0].view(F).reshape(-1, 8)
    assert R.same(rec[:, :3], R.mission_points(xyz, REF_POSE, read_pose)) and not rec[:, 4].any()
    cf.destroy()
    vis.destroy()


def test_unobserved_neighbours_yaw_near_pi_and_z(capi, ctx, pair16):
    """TSDF distances (unobserved beyond twice the truncation) under a 0.35 m offset: part of the points meet unobserved
    neighbours (the NaN sentinel path); yaw near +-pi on both poses and a non-zero z"""
    sm, g, xyz, dist = pair16
    w, factor = weights("quarters", len(xyz))
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS,
                                                                      use_esdf_distance=0, no_correspondence_cost=0.37))
    vis = capi.RegVisuals(ctx)
    layer = H.oracle_layer(sm, False)
    for ref_pose, read_pose in ((np.array([0.0, 0.0, 0.0, 0.0]), np.array([0.25, 0.2, 0.15, 0.02])),
                                (np.array([1.0, 2.0, 0.4, 3.1]), np.array([1.05, 1.97, 0.7, -3.12]))):
        ok, r, jo, je = gpu_eval(cf, vis, ref_pose, read_pose)
        rows = orc.reg_evaluate(layer, xyz, dist, w, ref_pose, read_pose, no_correspondence_cost=0.37)
        missing = ~rows[3].any(axis=1)
        assert ok and len(w) // 50 < missing.sum() < len(w) - len(w) // 50, missing.sum()
        check_against(vis, xyz, rows, factor, ref_pose, read_pose, "unobserved")
    cf.destroy()
    vis.destroy()


def test_gating_and_errors(capi, ctx, pair16):
    sm, g, xyz, dist = pair16
    w, factor = weights("ones", len(xyz))
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
    cf = capi.RegistrationCostFunction(ctx, g, g, cfg)
    vis = capi.RegVisuals(ctx)
    n = len(w)
    assert vis.stats() == (0, 0) and vis.device_pointers() == (None, None, None)
    # no Jacobians asked for: no markers, the cloud still filled
    ok, r, _, _ = gpu_eval(cf, vis, REF_POSE, READ_POSE, want_jac=False)
    assert ok and vis.stats() == (n, 0)
    full = vis.download()
    assert len(full[0]) == n and len(full[1]) == 0 and len(full[2]) == 0
    # ... and no gradients wanted
    ok, *_ = gpu_eval(cf, vis, REF_POSE, READ_POSE, gradients=False)
    assert ok and vis.stats() == (n, 0) and R.same(vis.download()[0], full[0])
    # no cloud wanted
    ok, *_ = gpu_eval(cf, vis, REF_POSE, READ_POSE, cloud=False)
    assert ok and vis.stats() == (0, n)
    p = vis.device_pointers()
    assert p[0] is None and p[1] and p[2]
    # a NULL or a foreign handle: refused, the handle keeps what it held
    with pytest.raises(capi.VgxError) as e:
        gpu_eval(cf, None, REF_POSE, READ_POSE)
    assert e.value.code == capi.ERR_INVALID and "NULL visuals" in str(e.value)
    other = capi.Context(0)
    foreign = capi.RegVisuals(other)
    with pytest.raises(capi.VgxError) as e:
        gpu_eval(cf, foreign, REF_POSE, READ_POSE)
    assert e.value.code == capi.ERR_INVALID and "another context" in str(e.value)
    assert foreign.stats() == (0, 0) and vis.stats() == (0, n)
    foreign.destroy()
    other.close()
    # reused from a large n to a small n
    small = capi.RegistrationCostFunction
    g2 = H.gpu_submap(capi, ctx, sm, 32)
    g2.set_points(capi.POINTS_VOXELS, xyz[:7], dist[:7], w[:7])
    cf2 = small(ctx, g2, g, cfg)
    ok, *_ = gpu_eval(cf2, vis, REF_POSE, READ_POSE)
    assert ok and vis.stats() == (7, 7)
    cloud, arrows, origins, _ = vis.download()
    assert cloud.shape == (7, 32) and arrows.shape == (14, 3) and origins.shape == (7, 3)
    # all-zero weights: Evaluate returns false and the handle holds nothing
    g2.set_points(capi.POINTS_VOXELS, xyz[:7], dist[:7], np.zeros(7, F))
    cf3 = small(ctx, g2, g, cfg)
    ok, *_ = gpu_eval(cf3, vis, REF_POSE, READ_POSE)
    assert ok is False and vis.stats() == (0, 0)
    assert vis.download()[3] == 0.0
    # stale points: refused as in vgx_reg_evaluate
    with pytest.raises(capi.VgxError) as e:
        gpu_eval(cf2, vis, REF_POSE, READ_POSE)
    assert e.value.code == capi.ERR_INVALID and "were replaced" in str(e.value)
    with pytest.raises(capi.VgxError) as e0:
        cf2.Evaluate([REF_POSE, READ_POSE], np.zeros(7), None)
    assert "were replaced" in str(e0.value)
    for c in (cf, cf2, cf3):
        c.destroy()
    g2.destroy()
    vis.destroy()


def test_general_weights(capi, ctx, pair16):
    """A non-dyadic factor over >= 4 tiles (secondary: the dyadic fixtures bind).  rows / factor is within one f64 ulp of
    the unscaled value.  j is an f32 value and an f64 within an ulp of it narrows back to it, so the tips are exact.  r_u
    is a full f64: its f32 narrowing can land on the neighbouring float, and the scaled, rounded intensity is then
    within 2 f32 ulp."""
    sm, g, xyz, dist = pair16
    w = np.random.default_rng(9).uniform(0.2, 1.0, len(xyz)).astype(F)
    factor = R.factor_of(w)
    assert len(w) >= 4 * TILE and np.frexp(factor)[0] != 0.5
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    vis = capi.RegVisuals(ctx)
    ok, r, jo, je = gpu_eval(cf, vis, REF_POSE, READ_POSE)
    cloud, arrows, origins, f = vis.download()
    assert ok and f == factor
    want = R.visuals(xyz, r, je, factor, REF_POSE, READ_POSE)
    got_rec, want_rec = cloud.view(F).reshape(-1, 8), want[0].view(F).reshape(-1, 8)
    assert R.same(got_rec[:, :4], want_rec[:, :4]) and R.same(got_rec[:, 5:], want_rec[:, 5:])
    ulps = R.ulp_distance_f32(got_rec[:, 4], want_rec[:, 4])
    print("general weights: factor", factor, "rows", len(w), "inexact intensities", int((ulps > 0).sum()), "worst ulp",
          int(ulps.max()))
    assert (ulps <= 2).all()
    assert R.same(origins, want[2]) and R.same(arrows, want[1])
    cf.destroy()
    vis.destroy()
