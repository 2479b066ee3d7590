"""Scan localisation on the device (vgx_scan_registration_set_map / _evaluate_map / _refine_map / _score_poses / _localize)
against the restatement of tests/scan_localization_ref.py, bit for bit.  The restatement is fed the arrays DOWNLOADED from
the device submaps, so the device ESDF's known deviation from the queue plays no part.  `evaluate_map` on random posed
submaps (holes, invalid voxels, general-quaternion poses, vps 8 and 16, both layers, with and without the Huber loss, one
to three submaps; points inside, outside, on faces, non-finite; every size at which the partition takes another path; a
stride; host, device and vgx_scan sources), against scan-to-map registration where the two coincide, `score_poses` against
per-pose evaluations and the restatement, `refine_map` on seeded priors in the asymmetric room over three kinds of map,
`localize` on the full 4608-hypothesis grid, the no-eligible-pose answer, a submap destroyed while listed, released layers
and every refusal."""
import math

import numpy as np
import pytest

from oracle import synth
from tests import scan_localization_ref as R
from tests import scan_localization_scenes as S
from tests import scan_registration_ref as SR
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
# n = 0, one point, around a wave, around one trip of a workgroup's threads, around one workgroup's quota (the second
# partial), and where the partials pass the fold's 256 threads
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1]
DELTAS = ((0.0, 0.0, 0.0, 0.0), (0.03, -0.02, 0.01, 0.02), (-0.4, 0.3, 0.2, -1.3), (0.0, 0.0, 0.0, math.pi))
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], F)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want):
    """(out, n_terms, n_points_valid, n_candidates) of the library and of the restatement"""
    assert tuple(got[1:]) == tuple(want[1:]), (got[1:], want[1:])
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])


def _upload(ctx, sid, d):
    return capi.Submap(ctx, sid, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.esdf_distance,
                       d.esdf_observed)


def _downloaded(sm):
    """what the device submap holds, as the restatement's SubmapData"""
    td, tw, ed, eo = sm.download_layers(sm.vps)
    return synth.SubmapData(sm.voxel_size, sm.vps, sm.block_index(), td, tw, ed, eo, np.zeros(4))


def _reg(ctx, submaps, poses, cfg=None, **map_kw):
    """a handle with its map set -> (handle, restatement config, restatement map config)"""
    cfg = dict(cfg or dict(max_abs_distance_m=0.25))
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(**cfg))
    reg.set_map(submaps, poses, capi.scan_map_config(**map_kw))
    return reg, SR.config(**cfg), R.map_config(**map_kw)


@pytest.fixture(scope="module", params=[8, 16])
def random_scene(request, ctx):
    vps = request.param
    rng = np.random.default_rng(70 + vps)
    data, poses = S.random_submaps(rng, vps)
    submaps = [_upload(ctx, k, d) for k, d in enumerate(data)]
    held = [_downloaded(sm) for sm in submaps]
    T = S.random_pose(rng) if vps == 8 else np.array([math.cos(0.35), 0, 0, math.sin(0.35), 0.3, -0.2, 0.1], F)
    pc = S.sensor_points(rng, data, poses, 150000, T)
    assert len(pc) > max(SIZES)
    yield submaps, held, poses, T, pc
    for sm in submaps:
        sm.destroy()


def test_evaluate_map_at_every_size(ctx, random_scene):
    submaps, held, poses, T, pc = random_scene
    layer = "tsdf" if submaps[0].vps == 8 else "esdf"
    reg, cfg, mcfg = _reg(ctx, submaps[:2], poses[:2], layer=layer, huber_delta_m=0.3)
    M = R.Map(held[:2], poses[:2], layer)
    terms = R.map_terms(M, pc[:max(SIZES)], T, DELTAS[1], cfg, mcfg)
    for n in SIZES:
        reg.set_points(pc[:n])
        got = reg.evaluate_map(T, DELTAS[1])
        _same(got, R.totals(*terms, m=n))
        if n > 1000:
            assert 0 < got[2] < got[1] < 2 * got[2] and got[2] < got[3] < n   # some points in both submaps; every kind of cut
    # the number of candidates, not of points, decides the partition: stride 3 at the same thresholds
    cfg3 = dict(max_abs_distance_m=0.25, point_stride=3)
    reg3, rcfg3, _ = _reg(ctx, submaps[:2], poses[:2], cfg3, layer=layer, huber_delta_m=0.3)
    terms3 = R.map_terms(M, pc[:100000], T, DELTAS[1], rcfg3, mcfg)
    for n in (1, 2, 3, 4, 3 * 256, 3 * 256 + 1, 3 * 1024, 3 * 1024 + 1, 3 * 1024 + 4, 100000):
        reg3.set_points(pc[:n])
        _same(reg3.evaluate_map(T, DELTAS[1]), R.totals(*terms3, m=-(-n // 3)))
    reg.destroy()
    reg3.destroy()


def test_evaluate_map_over_layers_losses_submap_counts_and_corrections(ctx, random_scene):
    submaps, held, poses, T, pc = random_scene
    n, turn = 12000, 0
    for K in (1, 2, 3):
        for layer in ("esdf", "tsdf"):
            M = R.Map(held[:K], poses[:K], layer)
            for huber in (math.inf, 0.3):
                cfg = dict(max_abs_distance_m=0.45 if layer == "esdf" else 0.25, min_range_m=0.2, max_range_m=2.5)
                reg, rcfg, mcfg = _reg(ctx, submaps[:K], poses[:K], cfg, layer=layer, huber_delta_m=huber)
                reg.set_points(pc[:n])
                deltas = DELTAS if (K, huber) == (3, 0.3) else (DELTAS[turn % 4],)
                turn += 1
                for delta in deltas:
                    got = reg.evaluate_map(T, delta)
                    _same(got, R.evaluate_map(M, pc[:n], T, delta, rcfg, mcfg))
                    assert 0 < got[2] <= got[1] <= K * got[2] and got[3] < n
                    assert K == 1 or got[1] > got[2]
                reg.destroy()
    # a submap without a block listed before or after a real one: its table misses every lookup, so the sums, the counts
    # and the scores are the real submap's alone, bit for bit
    vox = submaps[0].vps ** 3
    none = capi.Submap(ctx, 30, submaps[0].voxel_size, submaps[0].vps, np.zeros((0, 3), np.int32), np.zeros((0, vox), F),
                       np.zeros((0, vox), F))
    for layer in ("esdf", "tsdf"):
        cfg = dict(max_abs_distance_m=0.45 if layer == "esdf" else 0.25)
        alone, _, _ = _reg(ctx, submaps[:1], poses[:1], cfg, layer=layer, huber_delta_m=0.3)
        alone.set_points(pc[:300])
        want, want_score = alone.evaluate_map(T, DELTAS[1]), alone.score_poses([T])
        assert want[1] > 0
        for listed, at in (([none, submaps[0]], [poses[1], poses[0]]), ([submaps[0], none], [poses[0], poses[1]])):
            reg, _, _ = _reg(ctx, listed, at, cfg, layer=layer, huber_delta_m=0.3)
            reg.set_points(pc[:300])
            _same(reg.evaluate_map(T, DELTAS[1]), want)
            assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(reg.score_poses([T]), want_score))
            reg.destroy()
        alone.destroy()
    none.destroy()


def test_host_device_and_scan_sources_agree(ctx, random_scene):
    import torch
    submaps, held, poses, T, pc = random_scene
    pts = pc[:5000][np.isfinite(pc[:5000]).all(1)]              # (a decoded scan holds finite points only)
    cfg = dict(max_abs_distance_m=0.25, point_stride=2)
    reg, rcfg, mcfg = _reg(ctx, submaps, poses, cfg, layer="esdf")
    want = R.evaluate_map(R.Map(held, poses, "esdf"), pts, T, DELTAS[1], rcfg, mcfg)
    reg.set_points(pts)
    _same(reg.evaluate_map(T, DELTAS[1]), want)
    dev = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    reg.set_points(dev)
    _same(reg.evaluate_map(T, DELTAS[1]), want)
    reg.set_points(dev.data_ptr(), len(pts))
    _same(reg.evaluate_map(T, DELTAS[1]), want)
    scan = capi.Scan(ctx)
    msg = pc[:5000].copy()                                       # the raw message: the decode drops the non-finite points
    layout = capi.scan_layout(width=len(msg), height=1, point_step=12, offset_x=0, offset_y=4, offset_z=8,
                              color_kind=capi.SCAN_COLOR_NONE)
    assert scan.decode_msg(layout, msg.tobytes())[0] == len(pts)
    reg.set_points(scan)
    _same(reg.evaluate_map(T, DELTAS[1]), want)
    reg.destroy()
    scan.destroy()


def test_score_poses_against_evaluations_and_the_restatement(ctx, random_scene):
    submaps, held, poses, T, pc = random_scene
    rng = np.random.default_rng(9)
    cfg = dict(max_abs_distance_m=0.25, point_stride=2)
    reg, rcfg, mcfg = _reg(ctx, submaps[:2], poses[:2], cfg, layer="esdf", huber_delta_m=0.2, score_point_stride=2)
    M = R.Map(held[:2], poses[:2], "esdf")
    # (n_poses, n): with stride 2, n = 2 x 262145 puts 257 partials under one pose -- past the fold's width
    for n_poses, n, n_ref in ((1, 2 * 1025, 1), (2, 2 * 64, 2), (300, 2 * 1025, 64), (3, 2 * 262145, 1)):
        pts = np.concatenate([pc, pc, pc, pc])[:n]
        hyp = np.array([S.compose(T, S.random_pose(rng, 0.2) * [1, 0.05, 0.05, 0.05, 1, 1, 1]) for _ in range(n_poses)], F)
        hyp[:, :4] /= np.linalg.norm(hyp[:, :4].astype(np.float64), axis=1)[:, None]
        reg.set_points(pts)
        cost, nt, nv, nc = reg.score_poses(hyp)
        assert (nc == nc[0]).all() and (nv > 0).all() and (nt >= nv).all() and len(set(cost.tolist())) == n_poses
        for m in range(n_poses):
            out, n_terms, n_valid, n_cand = reg.evaluate_map(hyp[m])
            assert np.array_equal(_bits(np.float64(cost[m])), _bits(np.float64(0.5 * out[0]))), m
            assert (nt[m], nv[m], nc[m]) == (n_terms, n_valid, n_cand)
        pick = rng.choice(n_poses, n_ref, replace=False)
        want = R.score_poses(M, pts, hyp[pick], rcfg, mcfg)
        assert np.array_equal(_bits(cost[pick]), _bits(want[0]))
        assert all(np.array_equal(g[pick], w) for g, w in zip((nt, nv, nc), want[1:]))
    assert reg.score_poses(np.zeros((0, 7), F))[0].shape == (0,)           # n_poses = 0 is VGX_OK
    reg.destroy()


# ---------------------------------------------------------------------------
# the asymmetric room
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(ctx):
    """three maps of the room: the restatement's arrays uploaded; the device's own submap (the reproducible integrator's
    layer finished on the device, its ESDF generated there); and that one again under a non-identity T_M_S"""
    layer = capi.TsdfLayer(ctx, SR.VOXEL_SIZE, SR.VPS)
    integrator = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for T, pts in S.room_scans():
        integrator.integratePointCloud(T, pts)
    own = capi.Submap.from_tsdf_layer(ctx, layer, 1)
    own.generate_esdf()
    uploaded = _upload(ctx, 0, S.room_submap())
    yield dict(layer=layer, uploaded=uploaded, own=own, held_uploaded=_downloaded(uploaded), held_own=_downloaded(own),
               scan=S.scan_to_localize())
    for x in (uploaded, own, integrator, layer):
        x.destroy()


def test_identity_tsdf_submap_is_scan_to_map_registration(ctx, room):
    """a submap finished from an integrated layer, identity pose, TSDF, no loss: out[15] of vgx_scan_registration_evaluate
    on that layer"""
    reg, _, _ = _reg(ctx, [room["own"]], [IDENTITY], dict(max_abs_distance_m=SR.MAX_ABS_DISTANCE), layer="tsdf")
    reg.set_points(room["scan"])
    for seed, delta in enumerate(DELTAS):
        T = SR.pose7(S.TRUE_POSE + np.random.default_rng(seed).uniform(-1, 1, 4) * SR.PRIOR_OFF)
        out, nv, nc = reg.evaluate(room["layer"], T, delta)
        got = reg.evaluate_map(T, delta)
        assert np.array_equal(_bits(got[0]), _bits(out)) and got[1:] == (nv, nv, nc) and nv > 100   # (a yaw 1.3 rad off keeps few)
    reg.destroy()


def _same_refinement(reg, got, want):
    T, usable, delta, S_ = got
    wT, wdelta, wS, whistory = want
    assert np.array_equal(_bits(T), _bits(wT)) and usable == bool(wS["usable"])
    assert np.array_equal(_bits(delta), _bits(wdelta)), (delta, wdelta)
    for key in ("usable", "termination", "num_iterations", "num_successful_steps", "num_evaluations", "num_factorization_failures",
                "n_candidates", "n_valid_first", "n_valid_last"):
        assert S_[key] == wS[key], (key, S_[key], wS[key])
    for key in ("initial_cost", "final_cost"):
        assert np.array_equal(_bits(np.float64(S_[key])), _bits(np.float64(wS[key]))), key
    history = reg.history()
    assert len(history) == len(whistory)
    for k, (h, wh) in enumerate(zip(history, whistory)):
        for key in ("cost", "trial_cost", "gain_ratio", "radius", "step_norm"):
            assert np.array_equal(_bits(np.float64(h[key])), _bits(np.float64(wh[key]))), (k, key, h[key], wh[key])
        assert (h["accepted"], h["factorization_failed"]) == (wh["accepted"], wh["factorization_failed"])


def test_refine_map_on_the_seeded_priors(ctx, room):
    posed = S.random_pose(np.random.default_rng(2), 1.0)
    for sm, held, T_M_S, layer, huber in ((room["uploaded"], room["held_uploaded"], IDENTITY, "esdf", math.inf),
                                          (room["own"], room["held_own"], IDENTITY, "esdf", 0.5),
                                          (room["own"], room["held_own"], posed, "tsdf", math.inf)):
        distance = S.MAX_ABS_DISTANCE if layer == "esdf" else SR.MAX_ABS_DISTANCE
        reg, rcfg, mcfg = _reg(ctx, [sm], [T_M_S], dict(max_abs_distance_m=distance), layer=layer, huber_delta_m=huber)
        reg.set_points(room["scan"])
        M = R.Map([held], [T_M_S], layer)
        for seed in range(6):
            prior = S.TRUE_POSE + np.random.default_rng(1000 + seed).uniform(-1, 1, 4) * SR.PRIOR_OFF
            T = S.compose(T_M_S, SR.pose7(prior))
            got = reg.refine_map(T)
            _same_refinement(reg, got, R.refine_map(M, room["scan"], T, rcfg, mcfg))
            assert got[1] and got[3]["termination_type"] == capi.CONVERGENCE
        reg.destroy()


def test_localize_on_the_full_grid(ctx, room):
    from tests.test_scan_localization_cpu import TRANSLATION_BOUND_M, YAW_BOUND_RAD
    cfg = dict(max_abs_distance_m=S.MAX_ABS_DISTANCE, min_valid_ratio=0.5)
    reg, rcfg, mcfg = _reg(ctx, [room["own"]], [IDENTITY], cfg, layer="esdf", score_point_stride=4)
    reg.set_points(room["scan"])
    M = R.Map([room["held_own"]], [IDENTITY], "esdf")
    poses = R.hypothesis_grid(S.GRID_X, S.GRID_Y, S.GRID_YAWS, S.GRID_Z)
    assert len(poses) == 4608
    scores = reg.score_poses(poses)
    want_scores = R.score_poses(M, room["scan"], poses, rcfg, mcfg)
    assert np.array_equal(_bits(scores[0]), _bits(want_scores[0]))
    assert all(np.array_equal(g, w) for g, w in zip(scores[1:], want_scores[1:]))
    best, T, usable, delta, summary = reg.localize(poses)
    wbest, wT, wdelta, wsummary, whistory = R.localize(M, room["scan"], poses, rcfg, mcfg, scores=want_scores)
    assert best == wbest
    _same_refinement(reg, (T, usable, delta, summary), (wT, wdelta, wsummary, whistory))
    assert np.array_equal(_bits(poses[best]), _bits(SR.pose7((S.EXPECTED_CELL[0], S.EXPECTED_CELL[1], S.GRID_Z, S.EXPECTED_CELL[2]))))
    err = SR.pose_error(T, S.TRUE_POSE)
    print(f"best {best}, refined error {err[0]:.6f} m {err[1]:.3e} rad")
    assert usable and err[0] <= TRANSLATION_BOUND_M and err[1] <= YAW_BOUND_RAD
    assert err[0] < 0.5 * SR.VOXEL_SIZE and err[1] < math.radians(0.5)
    reg.destroy()


def test_no_eligible_hypothesis_is_an_answer(ctx, room):
    reg, _, _ = _reg(ctx, [room["uploaded"]], [IDENTITY], dict(max_abs_distance_m=S.MAX_ABS_DISTANCE), score_point_stride=4)
    reg.set_points(room["scan"])
    assert reg.refine_map(SR.pose7(S.TRUE_POSE))[1] and len(reg.history()) > 0
    poses = R.hypothesis_grid([40.0, 41.0], [30.0], 4, 0.02)          # every hypothesis outside the room
    best, T, usable, delta, summary = reg.localize(poses)
    assert best == -1 and not usable and summary["termination_type"] == capi.FAILURE
    assert summary["termination_reason"] == capi.TERMINATION_TOO_FEW_POINTS and summary["num_evaluations"] == 0
    assert np.array_equal(_bits(T), _bits(poses[0])) and not delta.any() and reg.history() == []
    reg.destroy()


def test_a_submap_destroyed_while_listed_lives_until_the_map_lets_go(ctx, random_scene):
    _, held, poses, T, pc = random_scene
    a, b = _upload(ctx, 10, held[0]), _upload(ctx, 11, held[1])
    reg, rcfg, mcfg = _reg(ctx, [a, b, a], [poses[0], poses[1], poses[2]], layer="tsdf")
    reg.set_points(pc[:3000])
    want = R.evaluate_map(R.Map([held[0], held[1], held[0]], poses, "tsdf"), pc[:3000], T, DELTAS[1], rcfg, mcfg)
    a.destroy()                                                    # deferred: the handle lists it (twice)
    b.destroy()
    _same(reg.evaluate_map(T, DELTAS[1]), want)
    c = _upload(ctx, 12, held[2])
    reg.set_map([c], [poses[2]], capi.scan_map_config(layer="tsdf"))   # a and b go now
    _same(reg.evaluate_map(T, DELTAS[1]), R.evaluate_map(R.Map([held[2]], [poses[2]], "tsdf"), pc[:3000], T, DELTAS[1], rcfg, mcfg))
    c.destroy()
    _same(reg.evaluate_map(T, DELTAS[1]), R.evaluate_map(R.Map([held[2]], [poses[2]], "tsdf"), pc[:3000], T, DELTAS[1], rcfg, mcfg))
    reg.destroy()                                                  # ... and c with the handle


def test_released_and_never_generated_layers_are_refused(ctx, random_scene):
    _, held, poses, T, pc = random_scene
    d = held[0]
    sm = _upload(ctx, 20, d)
    no_esdf = capi.Submap(ctx, 21, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight)
    reg, _, _ = _reg(ctx, [sm, no_esdf], poses[:2], layer="esdf")
    reg.set_points(pc[:1000])
    for call in (lambda: reg.evaluate_map(T), lambda: reg.refine_map(T), lambda: reg.score_poses([T]), lambda: reg.localize([T])):
        with pytest.raises(capi.VgxError) as e:
            call()
        assert e.value.code == capi.ERR_INVALID and "not resident" in str(e.value)
    reg.set_map([sm, no_esdf], poses[:2], capi.scan_map_config(layer="tsdf"))
    assert reg.evaluate_map(T)[3] > 0
    sm.release_raw_layers()
    with pytest.raises(capi.VgxError) as e:
        reg.evaluate_map(T)
    assert e.value.code == capi.ERR_INVALID and "not resident" in str(e.value)
    for x in (reg, sm, no_esdf):
        x.destroy()


def test_refusals(ctx, random_scene):
    submaps, held, poses, T, pc = random_scene
    lib = ctx.lib
    C, f32p, f64p, i64p = capi.C, capi.f32p, capi.f64p, capi.i64p
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(0.25))

    def refused(fn, code=capi.ERR_INVALID):
        with pytest.raises(capi.VgxError) as e:
            fn()
        assert e.value.code == code, e.value

    # no map, then no points
    reg.set_points(pc[:100])
    for call in (lambda: reg.evaluate_map(T), lambda: reg.refine_map(T), lambda: reg.score_poses([T]), lambda: reg.localize([T])):
        refused(call)
    assert "no map" in lib.vgx_last_error(ctx.h).decode()
    fresh = capi.ScanRegistration(ctx, capi.scan_registration_config(0.25))
    fresh.set_map(submaps[:1], poses[:1])
    refused(lambda: fresh.evaluate_map(T))
    assert "no points" in lib.vgx_last_error(ctx.h).decode()
    fresh.destroy()

    # set_map: the configuration, the list, the poses
    for kw in (dict(layer=2), dict(layer=-1), dict(huber_delta_m=0.0), dict(huber_delta_m=-1.0), dict(huber_delta_m=math.nan),
               dict(score_point_stride=0)):
        refused(lambda: reg.set_map(submaps[:1], poses[:1], capi.scan_map_config(**kw)))
    other = capi.Context(0)
    foreign = _upload(other, 0, held[0])
    d = held[0]
    other_vps = 24 - d.vps
    nv = other_vps ** 3
    mixed = capi.Submap(ctx, 30, d.voxel_size, other_vps, d.block_index[:2], np.zeros((2, nv), F), np.ones((2, nv), F),
                        np.zeros((2, nv), F), np.ones((2, nv), np.uint8))
    bad_nan, bad_long = poses[:1].copy(), poses[:1].copy()
    bad_nan[0, 5] = np.nan
    bad_long[0, :4] *= F(1.0001)
    refused(lambda: reg.set_map([foreign], poses[:1]))
    refused(lambda: reg.set_map([submaps[0], mixed], poses[:2]))
    refused(lambda: reg.set_map([submaps[0]] * 65, np.tile(poses[:1], (65, 1))))
    refused(lambda: reg.set_map(submaps[:1], bad_nan))
    refused(lambda: reg.set_map(submaps[:1], bad_long))
    hs = (capi.vp * 1)(submaps[0].h)
    assert lib.vgx_scan_registration_set_map(reg.h, None, 1, None, capi._ptr(poses[:1], f32p)) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_map(reg.h, None, 1, hs, None) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_map(reg.h, None, -1, hs, capi._ptr(poses[:1], f32p)) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_map(None, None, 1, hs, capi._ptr(poses[:1], f32p)) == capi.ERR_INVALID
    assert lib.vgx_scan_registration_set_map(reg.h, None, 1, (capi.vp * 1)(None), capi._ptr(poses[:1], f32p)) == capi.ERR_INVALID
    refused(lambda: reg.evaluate_map(T))                                    # every refused set_map left no map
    reg.set_map([submaps[0]] * 64, np.tile(poses[:1], (64, 1)))             # 64 is allowed
    reg.set_map(submaps[:2], poses[:2])
    refused(lambda: reg.set_map([foreign], poses[:1]))                      # ... and a refused one leaves the map it found
    first = reg.evaluate_map(T)
    assert first[1] > 0
    reg.set_map([])                                                         # n_submaps = 0 clears it
    refused(lambda: reg.evaluate_map(T))
    reg.set_map(submaps[:2], poses[:2])

    # the calls: NULL arguments, poses, corrections; nothing written
    out, Tc, delta = np.full(15, 7.0), capi._f32(T), np.zeros(4)
    counts = [C.c_int64(-1) for _ in range(3)]
    Tr, dr, best = np.full(7, 7.0, F), np.full(4, 7.0), C.c_int32(7)
    cost = np.full(2, 7.0)

    def evaluate(T=Tc, delta=delta, out=out, h=reg.h):
        return lib.vgx_scan_registration_evaluate_map(h, capi._ptr(T, f32p), capi._ptr(delta, f64p), capi._ptr(out, f64p),
                                                      *[C.byref(c) for c in counts])

    def refine(T=Tc, Tr=Tr, dr=dr, h=reg.h):
        return lib.vgx_scan_registration_refine_map(h, capi._ptr(T, f32p), None, capi._ptr(Tr, f32p), capi._ptr(dr, f64p), None)

    def score(n=2, T=np.stack([Tc, Tc]), h=reg.h):
        return lib.vgx_scan_registration_score_poses(h, n, capi._ptr(T, f32p), capi._ptr(cost, f64p), None, None, None)

    def localize(n=2, T=np.stack([Tc, Tc]), best=best, Tr=Tr, dr=dr, h=reg.h):
        return lib.vgx_scan_registration_localize(h, n, capi._ptr(T, f32p), None, None if best is None else C.byref(best),
                                                  capi._ptr(Tr, f32p), capi._ptr(dr, f64p), None)

    nan_T, inf_T, long_T = Tc.copy(), Tc.copy(), Tc.copy()
    nan_T[5], inf_T[0] = np.nan, np.inf
    long_T[:4] *= F(1.0001)
    for rc in (evaluate(T=None), evaluate(delta=None), evaluate(out=None), evaluate(T=nan_T), evaluate(T=inf_T), evaluate(T=long_T),
               evaluate(delta=np.array([0, np.nan, 0, 0.0])), evaluate(delta=np.array([0, 0, 0, np.inf])), evaluate(h=None),
               refine(T=None), refine(Tr=None), refine(dr=None), refine(T=nan_T), refine(T=long_T), refine(h=None),
               score(n=-1), score(T=None), score(T=np.stack([Tc, nan_T])), score(T=np.stack([long_T, Tc])), score(h=None),
               localize(n=-1), localize(T=None), localize(best=None), localize(Tr=None), localize(dr=None),
               localize(T=np.stack([Tc, inf_T])), localize(h=None)):
        assert rc == capi.ERR_INVALID
    assert (out == 7.0).all() and (Tr == 7.0).all() and (dr == 7.0).all() and best.value == 7 and (cost == 7.0).all()
    assert [c.value for c in counts] == [-1, -1, -1]
    opts = capi.pose_graph_options(initial_trust_region_radius=0.0)
    assert lib.vgx_scan_registration_refine_map(reg.h, capi._ptr(Tc, f32p), C.byref(opts), capi._ptr(Tr, f32p), capi._ptr(dr, f64p),
                                                None) == capi.ERR_INVALID
    assert evaluate() == capi.OK and counts[2].value > 0 and np.array_equal(_bits(out), _bits(first[0]))
    # launches past 2^31 - 1 workgroups: refused before anything is read (addresses nobody dereferences)
    reg.set_points(1 << 20, (2 ** 31 - 1) * 1024 + 1)
    assert evaluate() == capi.ERR_UNSUPPORTED and refine() == capi.ERR_UNSUPPORTED and localize() == capi.ERR_UNSUPPORTED
    reg.set_points(1 << 20, 2 ** 30 * 1024)                                  # 2^30 slots per pose: two poses are too many
    assert score() == capi.ERR_UNSUPPORTED and localize() == capi.ERR_UNSUPPORTED
    for x in (reg, foreign, mixed):
        x.destroy()
    other.close()


def test_special_voxel_values_fall_under_the_stated_comparisons(ctx):
    """One point in the cube CELL of tests/special_voxel_scene.py's layer (D = Z0 - z, r = 0.0275 there) as a finished submap
    under the identity pose, the same field in its ESDF; a special value planted into CELL.  The expectations are IEEE's
    under the header's comparisons -- "TSDF weight > 0", "ESDF observed != 0", "|r| < max_abs_distance_m" -- written down
    by hand.  (An ESDF's validity is a byte: it has no special values.)"""
    from tests import special_voxel_scene as Z
    bi, d, w = Z.layer()
    seen = np.ones(d.shape, np.uint8)
    point = np.array([[Z.X, Z.Y, Z.Z_IN]], F)
    nb7, cell, other = [Z.NEIGHBOUR_7], Z.CELL, [Z.CELL[1]]

    def evaluate(layer, dd=d, ww=w):
        """(evaluate_map's result, score_poses' result) on a submap with these TSDF arrays, the distance in its ESDF too"""
        sm = capi.Submap(ctx, 0, Z.VOXEL_SIZE, Z.VPS, bi, dd, ww, dd, seen)
        reg, _, _ = _reg(ctx, [sm], [IDENTITY], dict(max_abs_distance_m=0.2), layer=layer)
        reg.set_points(point)
        got, score = reg.evaluate_map(IDENTITY), reg.score_poses([IDENTITY])
        reg.destroy()
        sm.destroy()
        assert score[0][0] == 0.5 * got[0][0] and (score[1][0], score[2][0], score[3][0]) == got[1:]
        return got

    def no_term(got):
        return got[1:] == (0, 0, 1) and not _bits(got[0]).any()                   # a candidate without a term; every sum +0

    for layer in ("tsdf", "esdf"):
        base = evaluate(layer)
        assert base[1:] == (1, 1, 1) and abs(base[0][0] - 0.0275 ** 2) < 1e-6 and abs(base[0][3] + 0.0275) < 1e-4
        # distance NaN, +inf, -inf (in neighbour 7 they reach r as they are; in another the inf meets its negation: NaN)
        # and 3e38: |r| < max_abs_distance_m fails: no term
        for where, value in ((nb7, np.nan), (nb7, np.inf), (nb7, -np.inf), (other, np.inf), (other, -np.inf), (nb7, 3e38), (cell, 3e38)):
            assert no_term(evaluate(layer, Z.plant(bi, d, where, value))), (layer, value)
        # -0.0, 0.0 and 1e-40 in one neighbour are ordinary values: the same bits from all three, not the unplanted ones
        sums = [evaluate(layer, Z.plant(bi, d, nb7, value)) for value in (-0.0, 0.0, 1e-40)]
        assert all(g[1:] == (1, 1, 1) for g in sums) and len({g[0].tobytes() for g in sums}) == 1 and sums[0][0][0] != base[0][0]
        # all 8 neighbours -0.0: r is a zero, |r| < max: a term, every sum a zero
        got = evaluate(layer, Z.plant(bi, d, cell, -0.0))
        assert got[1:] == (1, 1, 1) and not got[0].any()
        # all 8 neighbours 1e-40: r = 1e-40 exactly, a residual like any other: rho = r r, exact in f64 -- a device that
        # flushed denormals would give 0
        got = evaluate(layer, Z.plant(bi, d, cell, 1e-40))
        assert got[1:] == (1, 1, 1) and got[0][0] == float(F(1e-40)) ** 2 > 0 and not got[0][1:].any()
    # TSDF weights: 1e-40 (a denormal) and +inf are > 0, the sums those of weight 1; NaN, -0.0, 0.0, -1 are not: no term.
    # The ESDF reads `observed`, so there the same weights change nothing
    base = evaluate("tsdf")
    for value in Z.WEIGHTS_OBSERVED:
        got = evaluate("tsdf", ww=Z.plant(bi, w, nb7, value))
        assert got[1:] == (1, 1, 1) and np.array_equal(_bits(got[0]), _bits(base[0])), value
    for value in Z.WEIGHTS_UNOBSERVED:
        assert no_term(evaluate("tsdf", ww=Z.plant(bi, w, nb7, value))), value
        assert evaluate("esdf", ww=Z.plant(bi, w, nb7, value))[1:] == (1, 1, 1)
