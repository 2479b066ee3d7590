"""The pose-graph solve's sequential restatement (tests/pose_graph_ref.py) against what the project already trusts: the
harness solver (harness/lm.py) on the CPU oracle backend, and numpy's Cholesky within Higham's backward-error bound.
Also the CPU half of the mutation checks: each wrong order gives other bits on the very inputs the GPU tests compare
bit for bit (tests/test_pose_graph_gpu.py), so a library built with that mutation cannot pass them."""
import numpy as np
import pytest

from harness import lm
from harness.backends import OracleBackend
from tests import helpers as H
from tests import pose_graph_ref as ref

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def spd_cases(n, seed=0):
    """B^T B + I from seeded integer-valued B, and the same with a graded diagonal 1e-6 ... 1e6 (symmetric scaling)"""
    rng = np.random.default_rng(1000 * n + seed)
    B = rng.integers(-3, 4, (n, n)).astype(np.float64)
    A = B.T @ B + np.eye(n)
    s = np.logspace(-3, 3, n)
    return {"integer": (A, rng.integers(-5, 6, n).astype(np.float64)),
            "graded": (A * np.outer(s, s) / (1.0 + np.abs(A).max()), rng.normal(0, 1, n))}


# n = 1, 2; one below, at and one above the first two panel edges (63 ... 129); trailing tiles (200, 516); 1100 = 17
# panels + 12 columns, where the substitutions' row loops (1024 rows per trip) take a second trip
SIZES = (1, 2, 4, 60, 63, 64, 65, 68, 127, 128, 129, 200, 516, 1100)


def lower_product(L, block=128):
    """the lower triangle of L L^T for a lower-triangular L, in longdouble: block (I, J <= I) sums over the columns below
    J's end only, which are all that both rows have -- a sixth of the full product's work, the same sums"""
    L = np.ascontiguousarray(L, np.longdouble)
    n = L.shape[0]
    P = np.zeros((n, n), np.longdouble)
    for i0 in range(0, n, block):
        for j0 in range(0, i0 + 1, block):
            k = min(j0 + block, n)
            P[i0:i0 + block, j0:j0 + block] = L[i0:i0 + block, :k] @ np.ascontiguousarray(L[j0:j0 + block, :k].T)
    return np.tril(P)


@pytest.mark.parametrize("n", SIZES)
def test_cholesky_restatement_within_highams_bound_and_next_to_numpys(n):
    """every comparison on the lower triangle: A, L L^T and the bounds are symmetric"""
    for name, (A, b) in spd_cases(n).items():
        assert np.array_equal(A, A.T)
        x, L = ref.spd_solve(A, b)
        Ln = np.linalg.cholesky(A)
        Al, Ll = np.tril(A).astype(np.longdouble), L.astype(np.longdouble)
        LLt, LnLnt = lower_product(L), lower_product(Ln)
        bound = gamma(n + 1) * lower_product(np.abs(L))
        assert np.all(np.abs(Al - LLt) <= bound), (name, n)
        # numpy's factor obeys the same bound, so the two products differ by no more than the sum of the two bounds
        bound_n = gamma(n + 1) * lower_product(np.abs(Ln))
        assert np.all(np.abs(LLt - LnLnt) <= bound + bound_n), (name, n)
        xl = x.astype(np.longdouble)
        assert np.all(np.abs(A.astype(np.longdouble) @ xl - b) <= gamma(3 * n + 1) * (np.abs(Ll) @ (np.abs(Ll).T @ np.abs(xl)))), (name, n)


def test_cholesky_restatement_refuses_what_is_not_positive_definite():
    A, _ = spd_cases(200)["integer"]
    for k in (0, 70, 199):
        for bad in (-1.0, np.nan):
            M = A.copy()
            M[k, k] = bad if np.isnan(bad) else -abs(M[k, k]) * 1e6
            with pytest.raises(ref.NotPositiveDefinite):
                ref.cholesky(M)


def test_summing_a_tiles_products_first_changes_the_factor():
    """mutation check, CPU half: products summed before the subtraction round differently at every size with a trailing tile"""
    for n in (68, 200, 516):
        A, _ = spd_cases(n)["graded"]
        assert not np.array_equal(ref.cholesky(A), ref.cholesky(A, sum_products_first=True)), n


@pytest.fixture(scope="module")
def ring():
    g = ref.ring_graph(12, seed=0)
    sms = ref.ring_submaps(g)
    g["backend"] = OracleBackend([H.oracle_layer(s) for s in sms], [H.oracle_points(s) for s in sms], g["pairs"], g["n"])
    return g


def _compare_with_harness(registration, backend, g, poses0, **kw):
    x, s, hist = ref.solve(registration, g["n"], g["constant"], g["edges"], poses0, max_solver_time_in_seconds=600, **kw)
    names = dict(max_num_iterations="max_iterations", initial_trust_region_radius="initial_radius")
    constant_nodes = [k for k in range(g["n"]) if g["constant"][k]]
    xh, sh = lm.solve(lm.Problem(backend, g["n"], g["pairs"], ref.lm_edges(g["edges"]), constant_nodes=constant_nodes), poses0,
                      max_seconds=600, **{names.get(k, k): v for k, v in kw.items()})
    rhos = [h["gain_ratio"] for h in hist if h["trial_cost"] != 0.0]
    print("restatement", s, "\nharness", {k: sh[k] for k in ("termination", "iterations", "final_cost")}, "\ngain ratios", rhos)
    assert rhos and min(abs(r - 1e-3) for r in rhos) > 1e-6        # the pinned seed keeps every decision off the threshold
    assert s["termination"] == sh["termination"] and s["num_iterations"] == sh["iterations"]
    assert [k + 1 for k, h in enumerate(hist) if h["accepted"]] == [it for it, _ in sh["cost_history"][1:]]
    dt = np.abs(x[:, :3] - xh[:, :3]).max()
    dyaw = np.abs(lm.normalize_angle(x[:, 3] - xh[:, 3])).max()
    print("restatement vs harness: dt", dt, "m, dyaw", dyaw, "rad")
    assert dt <= 1e-9 and dyaw <= 1e-9
    assert s["final_cost"] < s["initial_cost"]
    return x


def test_restatement_follows_the_harness_solver_on_a_ring_with_two_loop_closures(ring):
    _compare_with_harness(ref.BackendRegistration(ring["backend"], ring["pairs"]), ring["backend"], ring, ring["poses0"])


def test_restatement_follows_the_harness_solver_through_the_two_stage_optimise(ring):
    """pose_graph_interface.cpp:182-191: registration excluded first, then the full problem from that result"""
    zero = lm.zero_registration_backend(ring["n"], len(ring["pairs"]))
    x1 = _compare_with_harness(ref.ZeroRegistration(), zero, ring, ring["poses0"])
    _compare_with_harness(ref.BackendRegistration(ring["backend"], ring["pairs"]), ring["backend"], ring, x1)


def test_assembly_order_mutations_change_the_system():
    """mutation check, CPU half: contributions added in another order, or without the transpose at (b, a), give another H
    on the assembly test's graph shape (two mirrored constraints on one pair, a pair at the constant node, three edges)"""
    rng = np.random.default_rng(5)
    n, pairs = 6, [(1, 2), (2, 1), (0, 3), (3, 4), (4, 5), (2, 5)]
    fused = rng.normal(0, 1, 1 + 20 * n + 16 * len(pairs))
    poses = rng.normal(0, 1, (n, 4))
    edges = [(1, 2, rng.normal(0, 1, 3), 0.2, rng.normal(0, 1, (4, 4))), (0, 4, rng.normal(0, 1, 3), -0.1, np.eye(4)),
             (5, 2, rng.normal(0, 1, 3), 0.3, rng.normal(0, 1, (4, 4)))]
    terms = [ref.edge_terms(e, poses[e[0]], poses[e[1]]) for e in edges]
    const = [1, 0, 0, 0, 0, 0]
    H0, g0 = ref.assemble(n, const, pairs, fused, edges, terms)
    assert H0.shape == (20, 20)
    assert not np.array_equal(H0, ref.assemble(n, const, pairs, fused, edges, terms, swap_steps_2_and_3=True)[0])
    assert not np.array_equal(H0, ref.assemble(n, const, pairs, fused, edges, terms, drop_transpose=True)[0])
    # against the harness's own (vectorised) assembly, to rounding
    prob = lm.Problem(lambda p: fused, n, pairs, [], constant_nodes=(0,))
    _, gh, Hh = prob.evaluate(poses)
    Hz, gz = ref.assemble(n, const, pairs, fused, [], [])
    np.testing.assert_allclose(Hz, Hh[4:, 4:], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(gz, gh[4:], rtol=1e-13, atol=1e-13)


# ---- the mixed graph: several constant nodes, a hub, full sqrt-information matrices, yaws all around the circle -------
def test_mixed_graph_is_the_scene_the_gpu_tests_need():
    g = ref.mixed_graph(80, ref.MIXED_SEED)
    pos, nfree = ref.free_positions(80, g["constant"])
    assert nfree == 77 and [k for k in range(80) if g["constant"][k]] == [0, 26, 54]
    assert {pos[k] - k for k in range(80) if pos[k] >= 0} == {-1, -2, -3}            # never i - 1 alone
    hub = g["hub"]
    as_a = [e for e in g["edges"] if e[0] == hub and abs(e[1] - hub) > 1]
    as_b = [e for e in g["edges"] if e[1] == hub and abs(e[0] - hub) > 1]
    assert len(as_a) >= 15 and len(as_b) >= 15 and len({e[1] for e in as_a} | {e[0] for e in as_b}) >= 30
    for e in as_a + as_b:
        S = np.asarray(e[4])
        assert np.count_nonzero(S) == 16 and not np.array_equal(S, S.T)
    ends = [(e[0], e[1]) for e in g["edges"]]
    assert (10, 11) in ends and (11, 10) in ends
    assert any(g["constant"][a] and not g["constant"][b] for a, b in ends)
    assert np.abs(g["poses0"][:, 3]).max() > 2 * np.pi                               # the start yaws arrive unwrapped
    assert (np.abs(ref.unwrapped_yaw_errors(g, g["poses0"])) > np.pi).sum() >= 10
    assert np.abs(g["true"][:, :3]).max() < 10.0                                     # metres: |x| leaves parameter_tolerance room


def test_mixed_graph_solve_accepts_rejects_and_wraps():
    """the preconditions of the GPU test's bit comparison (test_mixed_graph_solve_is_the_restatement_bit_for_bit), on the
    restatement alone, so that a seed or scene change that empties that test fails here, without a GPU"""
    g = ref.mixed_graph(80, ref.MIXED_SEED)
    x, s, hist = ref.solve(ref.ZeroRegistration(), 80, g["constant"], g["edges"], g["poses0"], max_solver_time_in_seconds=600,
                           **ref.MIXED_SOLVE)
    check_mixed_history(g, s, hist)


def check_mixed_history(g, s, hist):
    tried = [h for h in hist if h["trial_cost"] != 0.0]
    print(s, "\ngain ratios", [h["gain_ratio"] for h in tried])
    assert sum(h["accepted"] for h in hist) >= 3 and sum(1 for h in tried if not h["accepted"]) >= 1
    assert min(abs(h["gain_ratio"] - 1e-3) for h in tried) > 1e-6
    assert (np.abs(ref.unwrapped_yaw_errors(g, g["poses0"])) > np.pi).any()
    assert s["termination"] in ("function_tolerance", "parameter_tolerance") and s["final_cost"] < s["initial_cost"]


def test_restatement_follows_the_harness_solver_on_the_mixed_graph_with_diagonal_matrices():
    """the harness solver takes diagonal information only: the mixed graph with every sqrt-information matrix replaced
    by its diagonal.  The only route by which ref.solve's bookkeeping for several constant nodes is trusted."""
    g = ref.mixed_graph(80, ref.MIXED_SEED)
    g["edges"] = [(a, b, t, yaw, np.diag(np.diag(S))) for a, b, t, yaw, S in g["edges"]]
    _compare_with_harness(ref.ZeroRegistration(), lm.zero_registration_backend(80, 0), g, g["poses0"], **ref.MIXED_SOLVE)


def _half_cost_longdouble(edge, pa, pb):
    """0.5 |S e|^2 in numpy.longdouble, vectorised: not the restatement's loops"""
    ld = np.longdouble
    _, _, t_obs, yaw_obs, S = edge
    pa, pb, t_obs, S = np.asarray(pa, ld), np.asarray(pb, ld), np.asarray(t_obs, ld), np.asarray(S, ld).reshape(4, 4)
    pi = np.arctan(ld(1)) * 4
    c, s = np.cos(pa[3]), np.sin(pa[3])
    d = pb[:3] - pa[:3]
    yaw = pb[3] - pa[3] - ld(yaw_obs)
    e = np.array([c * d[0] + s * d[1] - t_obs[0], -s * d[0] + c * d[1] - t_obs[1], d[2] - t_obs[2],
                  yaw - 2 * pi * np.floor((yaw + pi) / (2 * pi))], ld)
    r = S @ e
    return ld(0.5) * (r @ r)


@pytest.mark.parametrize("yaw_error", (0.3, np.pi - 0.05, np.pi + 0.05, -np.pi + 0.05, -np.pi - 0.05, 3 * np.pi - 0.05,
                                       3 * np.pi + 0.05, -5 * np.pi - 0.05, 2 * np.pi + 0.3))
def test_edge_terms_gradient_is_the_central_difference_of_half_the_cost(yaw_error):
    """ga, gb of ref.edge_terms (full sqrt-information, the yaw error on either side of +-pi and turns away from it)
    against (f(p + h) - f(p - h)) / 2h of f = 0.5 cost in longdouble, h = 1e-4, 0.05 rad off the wrap's jump.

    The tolerance.  f = 0.5 e^T M e, M = S^T S.  e is LINEAR in every variable but yaw_a (the wrap is a - const away from
    its jump), so f is a quadratic there and the central difference has no truncation error.  In theta = yaw_a:
    e_xy = R(theta)^T d - t, so |e_xy^(k)| = |d_xy| for every k >= 1, and e_yaw' = -1, e_yaw'' = 0.  With
    f''' = e'''^T M e + 3 e''^T M e':  |f'''| <= |S|_2^2 (|d_xy| |e| + 3 |d_xy| sqrt(|d_xy|^2 + 1)) =: B3, |e| taken at
    its largest over [theta - h, theta + h]: |e(theta)| + h sqrt(|d_xy|^2 + 1).  Truncation: h^2 / 6 B3.
    Rounding, four orders below that: the f64 gradient's nested 4-term sums (3 gamma(4), against 1-norms up to 64 times
    the 2-norm bound G = |S|_2^2 sqrt(|d_xy|^2 + 1) |e| of |f'|) and the difference's 16 u_ld f / h: 1e-12 (G + f)."""
    rng = np.random.default_rng(17)
    h = np.longdouble(1e-4)
    for case in range(4):
        S = rng.normal(0, 3, (4, 4))
        pa, pb = rng.normal(0, 2, 4), rng.normal(0, 2, 4)
        t_obs, yaw_obs = rng.normal(0, 2, 3), rng.normal(0, 1)
        pb[3] = pa[3] + yaw_obs + yaw_error
        edge = (0, 1, t_obs, yaw_obs, S)
        assert abs(abs(ref.normalize_angle(pb[3] - pa[3] - yaw_obs)) - np.pi) > 0.04          # h away from the jump
        cost, ga, gb = ref.edge_terms(edge, pa, pb)[:3]
        f0 = _half_cost_longdouble(edge, pa, pb)
        assert abs(0.5 * cost - float(f0)) <= 1e-13 * float(f0)
        dxy = float(np.hypot(pb[0] - pa[0], pb[1] - pa[1]))
        e_norm = np.sqrt(2.0 * float(f0)) / np.linalg.svd(S, compute_uv=False)[-1]            # |e| <= |S e| / sigma_min
        s2 = np.linalg.norm(S, 2) ** 2
        G = s2 * np.sqrt(dxy ** 2 + 1.0) * e_norm
        B3 = s2 * (dxy * (e_norm + float(h) * np.sqrt(dxy ** 2 + 1.0)) + 3.0 * dxy * np.sqrt(dxy ** 2 + 1.0))
        rounding = 1e-12 * (G + float(f0))
        for which, grad in ((0, ga), (1, gb)):
            for k in range(4):
                lo = [np.asarray(pa, np.longdouble).copy(), np.asarray(pb, np.longdouble).copy()]
                hi = [lo[0].copy(), lo[1].copy()]
                lo[which][k] -= h
                hi[which][k] += h
                fd = (_half_cost_longdouble(edge, *hi) - _half_cost_longdouble(edge, *lo)) / (2 * h)
                tol = rounding + (float(h) ** 2 / 6.0 * B3 if (which, k) == (0, 3) else 0.0)
                err = abs(float(np.longdouble(grad[k]) - fd))
                print(f"yaw error {yaw_error:+.3f} case {case} d f / d p{'ab'[which]}[{k}]: {grad[k]:+.6e}, off by {err:.2e}, tol {tol:.2e}")
                assert err <= tol, (case, which, k, err, tol)


def test_assembly_mutations_change_the_system_of_the_mixed_graph():
    """mutation checks, CPU half, on the GPU assembly test's graph (ref.assembly_scene: 80 nodes, three of them constant,
    the hub, a pair with two edges and two registration constraints): the two order mutations give another H, and so does
    a block row taken from the node index where the free position belongs; the right H against the harness's assembly"""
    g, ring, pairs, poses = ref.assembly_scene()
    n, const, edges = 80, g["constant"], g["edges"]
    fused = np.random.default_rng(6).normal(0, 1, 1 + 20 * n + 16 * len(pairs))
    terms = [ref.edge_terms(e, poses[e[0]], poses[e[1]]) for e in edges]
    H0, g0 = ref.assemble(n, const, pairs, fused, edges, terms)
    assert H0.shape == (308, 308)
    assert not np.array_equal(H0, ref.assemble(n, const, pairs, fused, edges, terms, swap_steps_2_and_3=True)[0])
    assert not np.array_equal(H0, ref.assemble(n, const, pairs, fused, edges, terms, drop_transpose=True)[0])
    # rows by node index: the system of a graph whose constant nodes all come first is another one
    first = [1, 1, 1] + [0] * 77
    assert not np.array_equal(H0, ref.assemble(n, first, pairs, fused, edges, terms)[0])
    touched = ref.touched_blocks(n, const, pairs, edges)
    assert 77 < touched.sum() < 77 * 77 // 4
    assert not H0[~np.kron(touched, np.ones((4, 4), bool))].any()
    prob = lm.Problem(lambda p: fused, n, pairs, ref.lm_edges([(a, b, t, yaw, np.diag(np.diag(S))) for a, b, t, yaw, S in edges]),
                      constant_nodes=(0, 26, 54))
    _, gh, Hh = prob.evaluate(poses)
    free = prob.free
    diag_terms = [ref.edge_terms((a, b, t, yaw, np.diag(np.diag(S))), poses[a], poses[b]) for a, b, t, yaw, S in edges]
    Hz, gz = ref.assemble(n, const, pairs, fused, edges, diag_terms)
    scale = np.abs(Hz).max()
    np.testing.assert_allclose(Hz, Hh[np.ix_(free, free)], rtol=1e-12, atol=1e-13 * scale)
    np.testing.assert_allclose(gz, gh[free], rtol=1e-12, atol=1e-13 * np.abs(gz).max())
