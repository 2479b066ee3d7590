"""Scan localisation on the CPU: the restatement of tests/scan_localization_ref.py checked on its own -- its Jacobian
against central differences of an f64 run (posed submap included), its agreement bit for bit with
tests/scan_registration_ref.py where the two formulations coincide, the Huber weights, two copies of one submap, the scoring
against the evaluation, and the whole recipe on the asymmetric room: 4608 hypotheses scored, the best one refined.  The
bounds are the measured figures of DESIGN.md 33."""
import math

import numpy as np
import pytest

from tests import scan_localization_ref as R
from tests import scan_localization_scenes as S
from tests import scan_registration_ref as SR

F = np.float32
SEEDS = range(6)
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], F)
# measured over SEEDS with this file (printed by the tests): the worst |J_f32 - central difference| was 2.93e-5 (the yaw
# column, |J| up to 16.6, through two more f32 rotations than scan-to-map registration's 1.43e-5).  Asserted at 4 x.
JACOBIAN_TOLERANCE = 4 * 2.93e-5
# measured with this file on the full grid: the chosen hypothesis scores 0.023664 against the runner-up's 0.026336, and the
# ESDF refinement from it ends 0.027025 m and 5.57e-4 rad from the true pose.  Asserted at 2 x (the margin is for the cost's
# discontinuity where points enter and leave observed space), and in any case below half a voxel and half a degree.
TRANSLATION_BOUND_M = 2 * 0.027025
YAW_BOUND_RAD = 2 * 5.57e-4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def room():
    return S.room_submap(), S.scan_to_localize()


def test_jacobian_against_central_differences_of_the_f64_formulas(room):
    sm, pts = room
    cfg, mcfg = SR.config(S.MAX_ABS_DISTANCE), R.map_config()
    worst = 0.0
    zero = [0.0] * 4
    for seed in SEEDS:
        rng = np.random.default_rng(300 + seed)
        T_M_S = S.random_pose(rng, 1.0)                      # the room, posed in the mission frame by a general quaternion
        M = R.Map([sm], [T_M_S], "esdf")
        prior = S.TRUE_POSE + rng.uniform(-1, 1, 4) * SR.PRIOR_OFF
        T = S.compose(T_M_S, SR.pose7(prior))
        _, [(usable, _, _)] = R.point_terms_map(M, pts, T, zero, cfg)
        # points kept well inside one interpolation cell, so that no step changes the 8 voxels read
        qi, ti = M.T_S_M[0]
        pm = R._mission_points(pts, T, zero, F)[1]
        _, _, dl = SR._neighbours(M.layers[0], (R.quat_rotate(qi, pm) + ti).astype(F), F)
        inner = usable & np.all([(x > 0.2) & (x < 0.8) for x in dl], 0)
        P = pts[inner]
        assert len(P) > 300
        _, [(u, _, J)] = R.point_terms_map(M, P, T, zero, cfg)
        assert u.all()
        h, cd = 1e-4, np.zeros((len(P), 4))
        for k in range(4):
            plus, minus = list(zero), list(zero)
            plus[k] += h
            minus[k] -= h
            _, [(up, rp, _)] = R.point_terms_map(M, P, T, plus, cfg, np.float64)
            _, [(um, rm, _)] = R.point_terms_map(M, P, T, minus, cfg, np.float64)
            assert up.all() and um.all()
            cd[:, k] = (rp - rm) / (2 * h)
        assert np.abs(cd).max(0).min() > 0.5                 # every column is exercised (a distance field: |grad D| ~ 1)
        dev = float(np.abs(J.astype(np.float64) - cd).max())
        print(f"seed {seed}: {len(P)} points, worst |J - central difference| = {dev:.3e}, |J| up to {np.abs(J).max():.2f}")
        worst = max(worst, dev)
    print(f"worst deviation {worst:.3e}, tolerance {JACOBIAN_TOLERANCE:.3e}")
    assert worst <= JACOBIAN_TOLERANCE


def test_one_identity_submap_without_loss_is_scan_to_map_registration(room):
    """K = 1, identity T_M_S, TSDF, Huber +inf: the bits of scan_registration_ref.evaluate on the same arrays"""
    sm, pts = room
    L = SR.layer_of(sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight)
    M = R.Map([sm], [IDENTITY], "tsdf")
    for stride, delta in ((1, (0.0, 0.0, 0.0, 0.0)), (1, (0.03, -0.02, 0.01, 0.02)), (3, (-0.2, 0.1, 0.05, -0.4))):
        cfg = SR.config(SR.MAX_ABS_DISTANCE, point_stride=stride)
        T = SR.pose7(S.TRUE_POSE + np.array([0.1, -0.1, 0.05, 0.02]))
        want, nv, nc = SR.evaluate(L, pts, T, delta, cfg)
        out, n_terms, n_valid, n_cand = R.evaluate_map(M, pts, T, delta, cfg, R.map_config(layer="tsdf"))
        assert np.array_equal(_bits(out), _bits(want)) and (n_terms, n_valid, n_cand) == (nv, nv, nc) and nv > 100


def test_huber_above_every_residual_is_no_loss_and_is_continuous(room):
    sm, pts = room
    M = R.Map([sm], [IDENTITY], "esdf")
    cfg, T = SR.config(S.MAX_ABS_DISTANCE), SR.pose7(S.TRUE_POSE + np.array([0.3, -0.2, 0.0, 0.1]))
    plain = R.evaluate_map(M, pts, T, [0.0] * 4, cfg, R.map_config())
    above = R.evaluate_map(M, pts, T, [0.0] * 4, cfg, R.map_config(huber_delta_m=S.MAX_ABS_DISTANCE))   # |r| < 1.9 at every term
    assert np.array_equal(_bits(plain[0]), _bits(above[0])) and plain[1:] == above[1:]
    robust = R.evaluate_map(M, pts, T, [0.0] * 4, cfg, R.map_config(huber_delta_m=0.3))
    assert robust[1:] == plain[1:] and 0 < robust[0][0] < plain[0][0] and (robust[0][5:] != plain[0][5:]).any()
    # rho and w at |r| = a from both sides: equal at a, within a few ulp one ulp beyond it
    for a in (F(0.3), F(0.05), F(1.0)):
        for sign in (1.0, -1.0):
            inside, outside = np.float64(a) * sign, np.nextafter(np.float64(a), np.inf) * sign
            (rho_in, rho_out), (w_in, w_out) = R.huber(np.array([inside, outside]), a)
            assert w_in == 1.0 and rho_in == float(a) * float(a)
            assert 0 < 1.0 - w_out < 1e-15 and abs(rho_out - rho_in) < 1e-15


def test_two_copies_of_one_submap_double_the_terms(room):
    sm, pts = room
    cfg, T = SR.config(S.MAX_ABS_DISTANCE), SR.pose7(S.TRUE_POSE + np.array([0.1, 0.1, 0.0, 0.05]))
    n = 900                                                 # one slot: a thread's sums are t + t per trip, then exact doubles
    one = R.evaluate_map(R.Map([sm], [IDENTITY]), pts[:n], T, [0.0] * 4, cfg, R.map_config(huber_delta_m=0.3))
    two = R.evaluate_map(R.Map([sm, sm], [IDENTITY, IDENTITY]), pts[:n], T, [0.0] * 4, cfg, R.map_config(huber_delta_m=0.3))
    assert two[1] == 2 * one[1] > 0 and two[2] == one[2] and two[3] == one[3]
    # with at most one trip per thread (n <= 256) every sum is (t + t) folded: exactly twice; beyond that to rounding
    small_one = R.evaluate_map(R.Map([sm], [IDENTITY]), pts[:256], T, [0.0] * 4, cfg, R.map_config())
    small_two = R.evaluate_map(R.Map([sm, sm], [IDENTITY, IDENTITY]), pts[:256], T, [0.0] * 4, cfg, R.map_config())
    assert np.array_equal(_bits(small_two[0]), _bits(2.0 * small_one[0]))
    assert np.allclose(two[0], 2.0 * one[0], rtol=1e-12, atol=0.0)


def test_scoring_is_the_evaluation_at_zero_correction(room):
    sm, pts = room
    rng = np.random.default_rng(5)
    T_M_S = [IDENTITY, S.random_pose(rng, 0.5)]
    M = R.Map([sm, sm], T_M_S, "esdf")
    cfg = SR.config(S.MAX_ABS_DISTANCE, point_stride=3)
    mcfg = R.map_config(huber_delta_m=0.5, score_point_stride=3)
    poses = np.array([SR.pose7(S.TRUE_POSE + rng.uniform(-1, 1, 4) * [1.0, 1.0, 0.05, 0.5]) for _ in range(5)], F)
    cost, nt, nv, nc = R.score_poses(M, pts, poses, cfg, mcfg, chunk=2)
    for m, T in enumerate(poses):
        out, n_terms, n_valid, n_cand = R.evaluate_map(M, pts, T, [0.0] * 4, cfg, mcfg)
        assert np.array_equal(_bits(np.float64(cost[m])), _bits(np.float64(0.5 * out[0])))
        assert (nt[m], nv[m], nc[m]) == (n_terms, n_valid, n_cand) and n_terms > n_valid > 100


def test_localisation_on_the_asymmetric_room(room):
    """the whole recipe: 32 x 12 x 24 hypotheses half a metre and 15 degrees apart, scored on every fourth point; the lowest
    mean cost among those with at least half their points usable; one ESDF refinement from it"""
    sm, pts = room
    M = R.Map([sm], [IDENTITY], "esdf")
    cfg, mcfg = SR.config(S.MAX_ABS_DISTANCE, min_valid_ratio=0.5), R.map_config(score_point_stride=4)
    poses = R.hypothesis_grid(S.GRID_X, S.GRID_Y, S.GRID_YAWS, S.GRID_Z)
    assert len(poses) == 4608
    scores = R.score_poses(M, pts, poses, cfg, mcfg)
    best, T, delta, summary, history = R.localize(M, pts, poses, cfg, mcfg, scores=scores)
    eligible = (scores[3] > 0) & (scores[2] / np.maximum(scores[3], 1) >= 0.5)
    mean = np.where(eligible, scores[0] / np.maximum(scores[1], 1), np.inf)
    order = np.argsort(mean, kind="stable")
    err = SR.pose_error(T, S.TRUE_POSE)
    print(f"{int(eligible.sum())} eligible of {len(poses)}; best {best} {poses[best][4:6]} score {mean[order[0]]:.6f}, runner-up "
          f"{mean[order[1]]:.6f}; refined error {err[0]:.6f} m {err[1]:.3e} rad ({summary['termination']}, "
          f"{summary['num_iterations']} iterations)")
    assert best == order[0] and 0 < eligible.sum() < len(poses)
    assert np.array_equal(_bits(poses[best]), _bits(SR.pose7((S.EXPECTED_CELL[0], S.EXPECTED_CELL[1], S.GRID_Z, S.EXPECTED_CELL[2]))))
    assert summary["usable"] == 1
    assert err[0] <= TRANSLATION_BOUND_M and err[1] <= YAW_BOUND_RAD
    assert err[0] < 0.5 * SR.VOXEL_SIZE and err[1] < math.radians(0.5)


def test_no_eligible_hypothesis_is_an_answer(room):
    sm, pts = room
    M = R.Map([sm], [IDENTITY], "esdf")
    cfg, mcfg = SR.config(S.MAX_ABS_DISTANCE), R.map_config(score_point_stride=4)
    poses = R.hypothesis_grid([40.0, 41.0], [30.0], 4, 0.02)          # every hypothesis outside the room
    best, T, delta, summary, history = R.localize(M, pts, poses, cfg, mcfg)
    assert best == -1 and summary["usable"] == 0 and summary["termination"] == SR.TOO_FEW_POINTS and history == []
    assert np.array_equal(_bits(T), _bits(poses[0])) and not delta.any()
