"""View rendering on the CPU: the restatement of tests/view_render_ref.py against analytic truth -- a single plane, whose
trilinear field is exact, and the box room of the scan-registration tests seen from the pose of its seventh scan -- and
the host-only part of the ABI: the two ray helpers, the config's defaults and every config refusal."""
import math

import numpy as np
import pytest

from tests import scan_registration_ref as R
from tests import view_render_ref as V
from voxgraph_amd import capi

F = np.float32


def test_a_plane_is_hit_where_it_is_observed_and_nowhere_else():
    """D = z - 0.3 over the block box [-3.2, 3.2]^3: 4000 downward rays from (0.13, -0.21, 2.1), seeded by where they meet
    the plane -- half of them at least a voxel inside the box's xy extent, half outside the box.  The band in between is
    left out of the seeding: an interpolation needs all 8 neighbours, so a ray ending in the outer half of the rim voxel
    misses and one ending in its inner half hits; 200 rays there are checked to be either, never INSIDE.
    Measured: 2089 hits, worst |range - truth| / truth = 8.1e-8."""
    bi, d, w = R.plane_layer(0.3)
    L = V.layer_of(R.VOXEL_SIZE, R.VPS, bi, d, w)
    cfg = V.config(s_max=10.0, min_step=0.05, unknown_step=0.2, max_bracket=0.6, step_scale=0.75)
    rng = np.random.default_rng(7)
    o = np.array([0.13, -0.21, 2.1])
    edge, vs = 3.2, R.VOXEL_SIZE
    inner = rng.uniform(-(edge - vs), edge - vs, (2000, 2))
    outer = rng.uniform(-6.0, 6.0, (6000, 2))
    outer = outer[np.abs(outer).max(1) > edge][:2000]
    rim = rng.uniform(-edge, edge, (4000, 2))
    rim = rim[(np.abs(rim).max(1) > edge - vs)][:200]
    assert len(outer) == 2000 and len(rim) == 200
    target = np.concatenate([np.concatenate([inner, outer, rim]), np.full((4200, 1), 0.3)], 1)
    to = target - o
    truth = np.linalg.norm(to, axis=1)
    dirs = (to / truth[:, None]).astype(F)
    assert (dirs[:, 2] < 0).all() and truth.max() < 10.0
    T = np.array([1, 0, 0, 0, *o], F)
    v = V.render(L, T, dirs, cfg)
    # where the f32 direction really meets the plane (the seeding is f64)
    truth = (0.3 - float(T[6])) / dirs[:, 2].astype(np.float64)
    at = np.abs(T[4:6].astype(np.float64) + dirs[:, :2].astype(np.float64) * truth[:, None]).max(1)
    inside, outside = at <= edge - vs, at > edge
    assert inside[:2000].all() and outside[2000:4000].all() and not (inside | outside)[4000:].any()
    assert (v.status[inside] == V.HIT).all()
    assert (v.status[outside] == V.MISS).all()
    assert np.isin(v.status[4000:], (V.HIT, V.MISS)).all() and not (v.status == V.INSIDE).any()
    hit = v.status == V.HIT
    err = np.abs(v.range[hit].astype(np.float64) - truth[hit]) / truth[hit]
    print(f"{int(hit.sum())} hits, worst relative range error {err.max():.3e}; mean samples {v.n_samples.mean():.1f}")
    assert err.max() <= 1e-6
    # at a hit: the point in the sensor frame, the plane's gradient (0, 0, 1) and weight 1; elsewhere zeros
    assert np.array_equal(v.points[hit], (dirs[hit] * v.range[hit][:, None]).astype(F))
    assert np.abs(v.gradient[hit] - np.array([0, 0, 1], F)).max() < 1e-4 and np.abs(v.weight[hit] - 1).max() < 1e-5
    for a in (v.range, v.points, v.gradient, v.weight):
        assert not a[~hit].any()
    assert v.counts["n_samples"] == int(v.n_samples.sum()) and v.counts["n_hit"] == int(hit.sum())
    assert (v.n_samples[hit] >= 3).all() and (v.n_samples >= 1).all()


def test_the_room_layer_seen_from_its_seventh_scan():
    """The CPU oracle's six-scan layer of the box room, rendered along room_scan's 256 x 16 beams from scan_pose(6) with
    a bracket of 0.65 m.  Measured with this file: hits 0.836 of the rays (0.809 HIT + 0.027 HIT_UNSAMPLED), MISS 0.038,
    INSIDE 0.126; |range - analytic room| over the hits: median 7.40 mm (7.15 mm over HIT alone), p99 0.189 m; 17.5 samples per ray, 59 at most.
    (A sparse LiDAR layer has unobserved bands next to its walls: with an unbounded bracket no ray ends INSIDE and 0.137
    of them are HIT_UNSAMPLED.)"""
    raw = R.room_layer()
    L = V.layer_of(R.VOXEL_SIZE, R.VPS, raw.bi, raw.d, raw.w)
    p4 = R.scan_pose(6)
    dirs = V.room_dirs()
    truth = np.linalg.norm(R.room_scan(p4).astype(np.float64), axis=1)
    v = V.render(L, R.pose7(p4), dirs, V.config(s_max=12.0, min_step=0.05, unknown_step=0.2, max_bracket=0.65))
    hit = (v.status == V.HIT) | (v.status == V.HIT_UNSAMPLED)
    err = np.abs(v.range[hit].astype(np.float64) - truth[hit])
    share = {k: float((v.status == s).mean()) for k, s in (("hit", V.HIT), ("unsampled", V.HIT_UNSAMPLED), ("miss", V.MISS),
                                                           ("inside", V.INSIDE))}
    print(f"shares {share}; range error median {np.median(err):.5f} m, p99 {np.percentile(err, 99):.4f} m; "
          f"samples mean {v.n_samples.mean():.2f} max {v.n_samples.max()}")
    assert hit.mean() >= 0.7
    assert np.median(err) <= R.VOXEL_SIZE / 10
    assert share["hit"] > 0 and share["miss"] > 0 and share["inside"] > 0
    assert not (v.status == V.BAD).any() and sum(v.counts[k] for k in V.COUNTS[1:6]) == len(dirs) == v.counts["n_rays"]
    # the gradient at a hit points back at the sensor: against the ray
    g = v.gradient[v.status == V.HIT].astype(np.float64)
    d_layer = R.quat_rotate(R.pose7(p4)[:4], dirs)[v.status == V.HIT].astype(np.float64)
    assert ((g * d_layer).sum(1) < 0).mean() > 0.99


def test_a_rendered_scan_registers_back_onto_its_layer():
    """scan -> layer -> scan: the view rendered at scan_pose(6) is a synthetic scan of the layer itself, so registering it
    from a prior 12 cm and 1 degree off must come back to the pose it was rendered at -- far closer than the real
    seventh scan does (1.3 cm), since the layer's own error cancels.  Rays without a hit are zero points:
    min_range_m > 0 leaves them out.  Measured: 3425 candidates, 3277 usable at the prior; 0.119 m / 0.0168 rad before,
    0.35 mm / 4.0e-6 rad after.  Asserted: a twentieth of a voxel (1 cm) and a hundredth of a degree."""
    raw = R.room_layer()
    L = V.layer_of(R.VOXEL_SIZE, R.VPS, raw.bi, raw.d, raw.w)
    truth = R.scan_pose(6)
    v = V.render(L, R.pose7(truth), V.room_dirs(), V.config(s_max=12.0, min_step=0.05, unknown_step=0.2, max_bracket=0.65))
    prior = R.pose7(R.seeded_prior(3))
    T, delta, S, _ = R.refine(raw, v.points, prior, R.config(R.MAX_ABS_DISTANCE, min_range_m=0.05))
    e0, e1 = R.pose_error(prior, truth), R.pose_error(T, truth)
    print(f"{S['n_candidates']} candidates, {S['n_valid_first']} usable; error {e0[0]:.4f} m {e0[1]:.5f} rad -> {e1[0]:.6f} m {e1[1]:.3e} rad")
    assert S["usable"] == 1 and S["n_candidates"] == v.counts["n_hit"] + v.counts["n_hit_unsampled"]
    assert e0[0] > 0.1 and e1[0] <= R.VOXEL_SIZE / 20 and e1[1] <= math.radians(0.01)


def test_bad_rays_the_start_and_the_reach():
    bi, d, w = R.plane_layer(0.3)
    L = V.layer_of(R.VOXEL_SIZE, R.VPS, bi, d, w)
    T = np.array([1, 0, 0, 0, 0.0, 0.0, 2.0], F)
    down = np.array([0, 0, -1], F)
    dirs = np.array([down, [0, 0, 0], [-0.0, 0, -0.0], [np.nan, 0, -1], [0, np.inf, -1], [0, 0, 1], F(0.5) * down], F)
    cfg = dict(s_max=8.0, min_step=0.05, unknown_step=0.2, max_bracket=0.6)
    v = V.render(L, T, dirs, V.config(**cfg))
    assert list(v.status) == [V.HIT, V.BAD, V.BAD, V.BAD, V.BAD, V.MISS, V.HIT]
    assert list(v.n_samples[1:5]) == [0, 0, 0, 0] and v.counts["n_bad"] == 4
    # s is in units of |dir|: a direction half as long doubles the range and keeps the point
    assert abs(v.range[0] - 1.7) < 1e-6 and abs(v.range[6] - 3.4) < 2e-6 and np.abs(v.points[0] - v.points[6]).max() < 1e-6
    # a reach short of the surface: MISS; a start behind it: INSIDE (the first valid sample is not positive)
    assert V.render(L, T, dirs[:1], V.config(**dict(cfg, s_max=1.5))).status[0] == V.MISS
    assert V.render(L, T, dirs[:1], V.config(**dict(cfg, s_min=2.0))).status[0] == V.INSIDE
    # a bracket narrower than the step that crosses the surface: INSIDE instead of a hit
    assert V.render(L, T, dirs[:1], V.config(**dict(cfg, max_bracket=0.01))).status[0] == V.INSIDE
    # an empty layer: every sample is invalid, every ray a MISS after s_max / unknown_step samples
    empty = V.layer_of(R.VOXEL_SIZE, R.VPS, np.zeros((0, 3), np.int32), np.zeros((0, R.VPS ** 3), F), np.zeros((0, R.VPS ** 3), F))
    v = V.render(empty, T, dirs[:1], V.config(**cfg))
    assert v.status[0] == V.MISS and v.n_samples[0] == 41


def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F))


def test_ray_helpers_against_numpy():
    """unit directions in f64, rounded once: within 1 f32 ulp of numpy (the libm may differ before the rounding)"""
    for w, h, fx, fy, cx, cy in ((640, 480, 525.0, 520.0, 319.5, 239.5), (7, 3, 4.0, -3.5, 2.2, 0.9), (1, 1, 1.0, 1.0, 0.0, 0.0)):
        got, want = capi.view_rays_pinhole(w, h, fx, fy, cx, cy), V.rays_pinhole(w, h, fx, fy, cx, cy)
        assert got.shape == (w * h, 3) and _ulps(got, want).max() <= 1
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-7
        # row-major [row][col]: the first row's x ascends with the column (fx > 0)
        assert w == 1 or (np.diff(got[:w, 0]) > 0).all()
    for w, h, lo, hi, off in ((1024, 64, -0.4, 0.3, 0.0), (256, 16, -0.296, 0.304, (2 * np.pi / 256) / 3.0), (5, 1, 0.1, 0.2, 1.0)):
        got, want = capi.view_rays_lidar(w, h, lo, hi, off), V.rays_lidar(w, h, lo, hi, off)
        assert got.shape == (w * h, 3) and _ulps(got, want).max() <= 1
    # room_scan's convention: the same beams
    got = capi.view_rays_lidar(256, 16, -0.296, 0.304, (2 * np.pi / 256) / 3.0)
    assert _ulps(got, V.room_dirs()).max() <= 1
    lib = capi.load()
    out = np.zeros(3, F)
    for rc in (lib.vgx_view_rays_pinhole(0, 1, 1.0, 1.0, 0.0, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_pinhole(1, 0, 1.0, 1.0, 0.0, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_pinhole(1, 1, 0.0, 1.0, 0.0, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_pinhole(1, 1, 1.0, math.nan, 0.0, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_pinhole(1, 1, 1.0, 1.0, 0.0, 0.0, None),
               lib.vgx_view_rays_lidar(0, 1, 0.0, 0.1, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_lidar(1, -1, 0.0, 0.1, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_lidar(1, 1, math.inf, 0.1, 0.0, capi._ptr(out, capi.f32p)),
               lib.vgx_view_rays_lidar(1, 1, 0.0, 0.1, 0.0, None)):
        assert rc == capi.ERR_INVALID
    assert not out.any()


def test_config_defaults():
    cfg = capi.ViewConfig()
    capi.load().vgx_view_config_default(capi.C.byref(cfg))
    assert (cfg.s_min, cfg.step_scale, cfg.image_width, cfg.flags) == (0.0, 0.75, 0, capi.VIEW_POINTS)
    # the four fields without a default are zero, and a zero is refused
    assert (cfg.s_max, cfg.min_step, cfg.unknown_step, cfg.max_bracket) == (0.0, 0.0, 0.0, 0.0)
    assert capi.view_config_check(cfg) == capi.ERR_INVALID
    good = capi.view_config(12.0, 0.05, 0.2, 0.6)
    assert capi.view_config_check(good) == capi.OK and abs(good.max_bracket - 0.6) < 1e-7
    assert capi.view_config_check(capi.view_config(12.0, 0.05, 0.2, 0.6, image_width=640, flags=capi.VIEW_ALL, s_min=12.0)) == capi.OK
    assert (capi.VIEW_MISS, capi.VIEW_HIT, capi.VIEW_INSIDE, capi.VIEW_BAD, capi.VIEW_HIT_UNSAMPLED) == (0, 1, 2, 3, 4)


GOOD = dict(s_max=12.0, min_step=0.05, unknown_step=0.2, max_bracket=0.6)
REFUSED = [dict(s_max=0.0), dict(min_step=0.0), dict(unknown_step=0.0), dict(max_bracket=0.0),
           dict(s_max=-1.0), dict(min_step=-0.05), dict(unknown_step=-0.2), dict(max_bracket=-0.6),
           dict(s_min=-0.001), dict(s_min=12.5), dict(step_scale=0.0), dict(step_scale=-0.75),
           dict(s_max=math.inf), dict(s_max=math.nan), dict(s_min=math.nan), dict(step_scale=math.inf), dict(min_step=math.nan),
           dict(unknown_step=math.inf), dict(max_bracket=math.inf), dict(max_bracket=math.nan),
           dict(s_max=3277.0),                                  # 3277 / 0.05 > 65536
           dict(min_step=1.0, unknown_step=12.0 / 65537),       # the smaller of the two steps counts
           dict(image_width=-1), dict(flags=32), dict(flags=-1), dict(flags=capi.VIEW_ALL + 32)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_config_refusals(kw):
    assert capi.view_config_check(capi.view_config(**dict(GOOD, **kw))) == capi.ERR_INVALID


def test_config_limits_and_null_arguments():
    assert capi.view_config_check(None) == capi.ERR_INVALID
    assert capi.view_config_check(capi.view_config(**dict(GOOD, s_max=3276.0))) == capi.OK       # 65520 samples at most
    assert capi.view_config_check(capi.view_config(**dict(GOOD, min_step=1.0, unknown_step=12.0 / 65535))) == capi.OK
    lib = capi.load()
    good, h = capi.view_config(**GOOD), capi.vp()
    # without a context nothing is created (and no device is touched)
    assert lib.vgx_view_create(None, capi.C.byref(good), capi.C.byref(h)) == capi.ERR_INVALID and not h.value
    assert lib.vgx_view_destroy(None) == capi.ERR_INVALID
    assert lib.vgx_view_stats(None, None) == capi.ERR_INVALID
    assert lib.vgx_view_download(None, None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_view_device_pointers(None, None, None, None, None, None, None, None) == capi.ERR_INVALID
    T, d = np.array([1, 0, 0, 0, 0, 0, 0], F), np.zeros(3, F)
    for fn in (lib.vgx_tsdf_layer_render_view, lib.vgx_submap_render_view):
        assert fn(None, None, capi._ptr(T, capi.f32p), 1, capi._ptr(d, capi.f32p)) == capi.ERR_INVALID
    for fn in (lib.vgx_tsdf_layer_render_view_device, lib.vgx_submap_render_view_device):
        assert fn(None, None, capi._ptr(T, capi.f32p), 1, None) == capi.ERR_INVALID
