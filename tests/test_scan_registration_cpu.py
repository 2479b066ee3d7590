"""Scan-to-map registration on the CPU: the restatement of tests/scan_registration_ref.py checked on its own -- its fold
against a lane-by-lane emulation of the partition, its Jacobian against central differences of an f64 run of the same
formulas, its recovery of a drifted prior on the box-room scene (the CPU oracle's layer), a single-plane layer, an
empty layer and an all-invalid scan.  The bounds are the measured figures of DESIGN.md 25."""
import math

import numpy as np
import pytest

from tests import scan_registration_ref as R

F = np.float32
SEEDS = range(6)
# measured over SEEDS with this file (printed by the tests): the worst |J_f32 - central difference| was 1.43e-5 (the yaw
# column, |J| up to 8); the worst end-pose error of the restatement 0.012643 m and 4.42e-4 rad.  Asserted: 4 x and 2 x.
JACOBIAN_TOLERANCE = 4 * 1.43e-5
TRANSLATION_BOUND_M = 2 * 0.012643
YAW_BOUND_RAD = 2 * 4.42e-4


@pytest.fixture(scope="module")
def room():
    return R.room_layer(), R.room_scan(R.scan_pose(6)), R.config(R.MAX_ABS_DISTANCE)


def _emulated_fold(terms):
    """the partition one lane at a time: candidate j to workgroup j / 1024, thread (j % 1024) % 256, trip (j % 1024) / 256"""
    def block(acc):                    # acc: 256 floats
        waves = []
        for w in range(4):
            v = list(acc[64 * w:64 * w + 64])
            o = 32
            while o > 0:
                for lane in range(o):
                    v[lane] = v[lane] + v[lane + o]
                o >>= 1
            waves.append(v[0])
        p = waves[0]
        for w in range(1, 4):
            p = p + waves[w]
        return p
    m = len(terms)
    partials = []
    for b in range(-(-m // 1024)):
        acc = [0.0] * 256
        for t in range(256):
            for trip in range(4):
                j = 1024 * b + 256 * trip + t
                if j < m:
                    acc[t] = acc[t] + float(terms[j])
        partials.append(block(acc))
    acc = [0.0] * 256
    for b, p in enumerate(partials):
        acc[b % 256] = acc[b % 256] + p
    return block(acc)


@pytest.mark.parametrize("m", [0, 1, 65, 257, 1023, 1025, 2500])
def test_fold_is_the_stated_partition(m):
    rng = np.random.default_rng(m)
    terms = (rng.normal(size=(m, 2)) * 10.0 ** rng.integers(-6, 6, (m, 2)))
    got = R.fold(terms)
    for k in range(2):
        want = _emulated_fold(terms[:, k]) if m else 0.0
        assert got[k] == want and (m < 2 or got[k] != 0.0)
    if m == 2500:                                           # the order is visible: another association gives other bits
        assert (got != terms.sum(0)).any() or (got != R.fold(terms, swap_partials=(0, 2))).any()


def test_fold_past_the_fold_width():
    """more partials than the fold has threads: partial b to thread b % 256, ascending"""
    m = 1024 * 258 + 3
    terms = np.random.default_rng(1).normal(size=(m, 1))
    assert R.fold(terms)[0] == _emulated_fold(terms[:, 0])


def test_jacobian_against_central_differences_of_the_f64_formulas(room):
    L, pts, cfg = room
    worst = 0.0
    for seed in SEEDS:
        T = R.pose7(R.seeded_prior(seed))
        zero = [0.0] * 4
        _, usable, _, _ = R.point_terms(L, pts, T, zero, cfg)
        # points kept well inside one interpolation cell, so that no step changes the 8 voxels read
        _, _, dl = R._neighbours(L, (R.quat_rotate(T[:4], pts) + T[4:]).astype(F), F)
        inner = usable & np.all([(x > 0.2) & (x < 0.8) for x in dl], 0)
        P = pts[inner]
        assert len(P) > 500
        _, u, _, J = R.point_terms(L, P, T, zero, cfg)
        assert u.all()
        h, cd = 1e-4, np.zeros((len(P), 4))
        for k in range(4):
            plus, minus = list(zero), list(zero)
            plus[k] += h
            minus[k] -= h
            _, up, rp, _ = R.point_terms(L, P, T, plus, cfg, np.float64)
            _, um, rm, _ = R.point_terms(L, P, T, minus, cfg, np.float64)
            assert up.all() and um.all()
            cd[:, k] = (rp - rm) / (2 * h)
        assert np.abs(cd).max(0).min() > 1.0                # every column is exercised
        dev = float(np.abs(J.astype(np.float64) - cd).max())
        print(f"seed {seed}: {len(P)} points, worst |J - central difference| = {dev:.3e}")
        worst = max(worst, dev)
    print(f"worst deviation {worst:.3e}, tolerance {JACOBIAN_TOLERANCE:.3e}")
    assert worst <= JACOBIAN_TOLERANCE


def test_recovery_on_the_box_room(room):
    L, pts, cfg = room
    truth = R.scan_pose(6)
    worst_t = worst_yaw = 0.0
    for seed in SEEDS:
        prior = R.seeded_prior(seed)
        T, delta, S, history = R.refine(L, pts, R.pose7(prior), cfg)
        share = S["n_valid_first"] / S["n_candidates"]
        e0, e1 = R.pose_error(R.pose7(prior), truth), R.pose_error(T, truth)
        print(f"seed {seed}: share {share:.3f}, {S['num_iterations']} iterations ({S['termination']}), "
              f"error {e0[0]:.4f} m {e0[1]:.5f} rad -> {e1[0]:.6f} m {e1[1]:.3e} rad, cost {S['final_cost']:.4f}")
        # every scene a test refines on: a usable share at its prior at or above the default min_valid_ratio
        assert S["n_candidates"] == len(pts) and share >= 0.5
        assert S["usable"] == 1 and S["num_evaluations"] == 1 + sum(1 for h in history if h["trial_cost"] != 0.0)
        assert S["final_cost"] < S["initial_cost"]
        worst_t, worst_yaw = max(worst_t, e1[0]), max(worst_yaw, e1[1])
    print(f"worst end-pose error {worst_t:.6f} m, {worst_yaw:.3e} rad")
    assert worst_t <= TRANSLATION_BOUND_M and worst_yaw <= YAW_BOUND_RAD


def test_a_single_plane_moves_only_what_it_observes():
    """D = z - z0: x, y and yaw are unobservable (their Jacobian columns are exactly zero); the solve neither fails nor
    moves them, and finds the height"""
    bi, d, w = R.plane_layer(0.3)
    L = R.layer_of(R.VOXEL_SIZE, R.VPS, bi, d, w)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-2.5, 2.5, (3000, 2)), np.full((3000, 1), 0.3 - 1.0)], 1).astype(F)   # the plane, seen from 1 m above
    prior = np.array([0.2, -0.1, 1.05, 0.4])                                                             # 5 cm too high
    T, delta, S, history = R.refine(L, pts, R.pose7(prior), R.config(R.MAX_ABS_DISTANCE))
    assert S["usable"] == 1 and S["num_factorization_failures"] == 0, S
    assert delta[0] == 0.0 and delta[1] == 0.0 and delta[3] == 0.0
    assert abs(delta[2] + 0.05) < 1e-5 and abs(float(T[6]) - 1.0) < 1e-5
    assert np.array_equal(T[[0, 1, 2, 3, 4, 5]].view(np.uint32), R.pose7(prior)[[0, 1, 2, 3, 4, 5]].view(np.uint32))


def test_an_empty_layer_and_an_all_invalid_scan_are_answers(room):
    L, pts, cfg = room
    prior = R.pose7(R.seeded_prior(0))
    empty = R.layer_of(R.VOXEL_SIZE, R.VPS, np.zeros((0, 3), np.int32), np.zeros((0, R.VPS ** 3), F), np.zeros((0, R.VPS ** 3), F))
    invalid = np.full((500, 3), np.nan, F)
    invalid[::3] = np.inf
    for layer, points, candidates in ((empty, pts, len(pts)), (L, invalid, len(invalid[::3])), (L, pts[:0], 0)):
        T, delta, S, history = R.refine(layer, points, prior, cfg)
        assert S["usable"] == 0 and S["num_iterations"] == 0 and history == [] and S["termination"] == R.TOO_FEW_POINTS
        assert S["n_candidates"] == candidates and S["n_valid_first"] == 0 and S["num_evaluations"] == 1
        assert np.array_equal(T.view(np.uint32), prior.view(np.uint32)) and not delta.any()


def test_range_and_stride_cut_candidates(room):
    L, pts, _ = room
    T = R.pose7(R.scan_pose(6))
    rng2 = (pts.astype(np.float64) ** 2).sum(1)
    cfg = R.config(R.MAX_ABS_DISTANCE, min_range_m=3.0, max_range_m=5.0, point_stride=3)
    out, nv, nc = R.evaluate(L, pts, T, [0.0] * 4, cfg)
    inside = (rng2[::3] > 9.001) & (rng2[::3] < 24.999)
    border = (np.abs(rng2[::3] - 9.0) < 2e-3) | (np.abs(rng2[::3] - 25.0) < 2e-3)
    assert inside.sum() <= nc <= inside.sum() + border.sum() and 0 < nv <= nc < len(pts[::3])
    # the sums at the true pose: residuals of a few centimetres, a positive definite H
    out, nv, nc = R.evaluate(L, pts, T, [0.0] * 4, R.config(R.MAX_ABS_DISTANCE))
    g, H = R.system(out)
    assert math.sqrt(out[0] / nv) < 0.05 and np.linalg.eigvalsh(H).min() > 0
