"""The edge covariances' sequential restatement (tests/pose_graph_covariance_ref.py) against what the project already
trusts: the backward-error bound of a Cholesky solve (Higham, Accuracy and Stability of Numerical Algorithms, theorem
10.4, in its componentwise form |A x - b| <= gamma(3n + 1) |L| |L^T| |x|, as tests/test_pose_graph_cpu.py uses it for one
right-hand side) and numpy's inverse.  Then the semantics of a block, and the CPU half of the mutation checks: each
wrong variant gives other bits on the very graph the GPU test compares bit for bit
(tests/test_pose_graph_covariance_gpu.py), so a library built with that mutation cannot pass it."""
import functools

import numpy as np
import pytest

from harness.backends import OracleBackend
from tests import helpers as H
from tests import pose_graph_covariance_ref as cov
from tests import pose_graph_ref as ref
from tests.test_pose_graph_cpu import gamma, spd_cases

LD = np.longdouble


@functools.lru_cache(maxsize=None)
def ring_system():
    """H of ref.ring_graph(12) at its start poses, registration (the CPU oracle backend) plus edges; nf = 44"""
    g = ref.ring_graph(12, seed=0)
    sms = ref.ring_submaps(g)
    backend = OracleBackend([H.oracle_layer(s) for s in sms], [H.oracle_points(s) for s in sms], g["pairs"], g["n"])
    fused, _ = ref.BackendRegistration(backend, g["pairs"]).full(g["poses0"])
    terms = [ref.edge_terms(e, g["poses0"][e[0]], g["poses0"][e[1]]) for e in g["edges"]]
    return g, ref.assemble(g["n"], g["constant"], g["pairs"], fused, g["edges"], terms)[0]


@functools.lru_cache(maxsize=None)
def mixed_system():
    """H of ref.mixed_graph(80) at its start poses; nf = 308, five panels"""
    g = ref.mixed_graph(80, ref.MIXED_SEED)
    return g, cov.assembled_system(g)[0]


def check_inverse(A, name):
    """X = solve_many(L, I): every column within the residual bound, and next to numpy's inverse.

    Residual: componentwise |A x_c - e_c| <= gamma(3n + 1) |L| |L^T| |x_c| =: d_c (the theorem, L the computed factor).
    Next to numpy: x_c - A^-1 e_c = A^-1 (A x_c - e_c), so |x_c - A^-1 e_c|_2 <= |A^-1|_2 |d_c|_2 = cond_2(A) / |A|_2
    |d_c|_2: the same bound scaled by the condition number.  numpy's inverse (LU with partial pivoting) carries an error
    of its own of that form, which is taken to be no larger: twice the bound."""
    n = A.shape[0]
    L = ref.cholesky(A)
    X = cov.solve_many(L, np.eye(n))
    Al, Xl, La = A.astype(LD), X.astype(LD), np.abs(L).astype(LD)
    bound = gamma(3 * n + 1) * (La @ (La.T @ np.abs(Xl)))
    residual = np.abs(Al @ Xl - np.eye(n, dtype=LD))
    assert np.all(residual <= bound), (name, n, float((residual / np.maximum(bound, LD(1e-300))).max()))
    s = np.linalg.svd(A, compute_uv=False)
    inverse_norm = 1.0 / s[-1]                                      # = cond_2(A) / |A|_2
    off = np.linalg.norm(X - np.linalg.inv(A), axis=0)
    allowed = 2.0 * inverse_norm * np.linalg.norm(bound.astype(np.float64), axis=0)
    print(f"{name} n {n}: cond {s[0] / s[-1]:.2e}, max residual / bound {float((residual / np.maximum(bound, LD(1e-300))).max()):.3f}, "
          f"max |x_c - numpy's| / allowed {(off / allowed).max():.3e}")
    assert np.all(off <= allowed), (name, n)
    return X


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 129, 200))
def test_solve_many_within_the_backward_error_bound_and_next_to_numpys_inverse(n):
    for name, (A, _) in spd_cases(n).items():
        check_inverse(A, name)


def test_solve_many_is_forward_and_backward_of_every_column():
    A, _ = spd_cases(129)["graded"]
    rng = np.random.default_rng(4)
    B = rng.normal(0, 1, (129, 7))
    B[:, 2] = 0.0
    B[:, 5] = np.eye(129)[:, 70]
    L = ref.cholesky(A)
    X = cov.solve_many(L, B)
    for c in range(7):
        assert np.array_equal(X[:, c].view(np.uint64), ref.backward(L, ref.forward(L, B[:, c])).view(np.uint64)), c
    assert not X[:, 2].any() and not np.signbit(X[:, 2]).any()      # +0.0 stays +0.0 through both passes


def test_covariances_of_the_ring_and_the_mixed_graph_within_the_bound():
    for name, (g, Hs) in (("ring", ring_system()), ("mixed", mixed_system())):
        assert np.array_equal(Hs, Hs.T)
        X = check_inverse(Hs, name)
        pos, nfree = ref.free_positions(g["n"], g["constant"])
        free = [k for k in range(g["n"]) if pos[k] >= 0]
        pairs = [(a, b) for a in free[:6] for b in free[-6:]]
        blocks = cov.covariance_blocks(Hs, g["n"], g["constant"], pairs)
        for p, (a, b) in enumerate(pairs):                              # a block IS that part of the solved inverse
            assert np.array_equal(blocks[p], X[4 * pos[a]:4 * pos[a] + 4, 4 * pos[b]:4 * pos[b] + 4])


def test_block_semantics():
    g, Hs = mixed_system()
    n, const, hub = g["n"], g["constant"], g["hub"]
    pairs = [(hub, 40), (40, hub), (0, hub), (hub, 26), (54, 0), (hub, hub), (hub, 40), (79, 1)]
    blocks = cov.covariance_blocks(Hs, n, const, pairs)
    assert blocks.shape == (8, 4, 4)
    for p in (2, 3, 4):                                                 # a constant node: sixteen zeros
        assert not blocks[p].any()
    assert np.array_equal(blocks[0], blocks[6])                         # duplicates are equal
    assert all(np.abs(blocks[p]).min() > 0 for p in (0, 1, 5, 7))
    # (a, b) and the transpose of (b, a): the same block of the exact inverse, each within the forward-error bound of
    # check_inverse -- 2 |H^-1|_2 max_c |d_c|_2 apart at the most, and not required to agree in bits
    L = ref.cholesky(Hs)
    X = cov.solve_many(L, np.eye(len(Hs)))
    La = np.abs(L)
    d = gamma(3 * len(Hs) + 1) * np.linalg.norm(La @ (La.T @ np.abs(X)), axis=0).max()
    allowed = 2.0 * d / np.linalg.svd(Hs, compute_uv=False)[-1]
    apart = np.abs(blocks[0] - blocks[1].T).max()
    print(f"(a, b) against (b, a)^T: {apart:.3e} apart, allowed {allowed:.3e}, block scale {np.abs(blocks[0]).max():.3e}")
    assert apart <= allowed
    # all nodes constant: zeros, nothing factorised
    assert not cov.covariance_blocks(np.zeros((0, 0)), 3, [1, 1, 1], [(0, 1), (2, 2)]).any()


def untouched_node_graph():
    """6 nodes in a chain, node 0 constant, node 4 left out of every edge: its diagonal block of H is zero"""
    g = cov.chain_graph(6, seed=1)
    g["edges"] = [e for e in g["edges"] if 4 not in (e[0], e[1])]
    return g


def test_a_node_no_constraint_touches_raises():
    g = untouched_node_graph()
    Hs = cov.assembled_system(g)[0]
    assert len(g["edges"]) >= 4 and not Hs[12:16].any()
    with pytest.raises(cov.NotPositiveDefinite) as e:
        cov.covariance_blocks(Hs, 6, g["constant"], [(1, 2)])
    assert e.value.args[0] == 12
    g = cov.chain_graph(6, seed=1)                                      # ... and with its edges it does not
    assert np.isfinite(cov.covariance_blocks(cov.assembled_system(g)[0], 6, g["constant"], [(1, 2), (4, 4)])).all()


def mutation_pairs(g):
    hub = g["hub"]
    hub_pairs = [(e[0], e[1]) for e in g["edges"] if hub in (e[0], e[1]) and abs(e[0] - e[1]) > 1]
    return hub_pairs + [(10, 11), (11, 10), (0, hub), (hub, 26), (54, 54)]


def test_mutations_change_the_bits_on_the_mixed_graph():
    """mutation checks, CPU half: a panel's products summed before the subtraction; (a, b) served as the transpose of
    (b, a); damping added (the solve's H + diag(H) / radius at the first radius, 1e4)"""
    g, Hs = mixed_system()
    pairs = mutation_pairs(g)
    assert len(pairs) >= 36
    right = cov.covariance_blocks(Hs, 80, g["constant"], pairs)
    pos, _ = ref.free_positions(80, g["constant"])
    L = ref.cholesky(Hs)
    seconds = sorted({pos[b] for a, b in pairs if pos[a] >= 0 and pos[b] >= 0})
    B = np.zeros((308, 4 * len(seconds)))
    for k, b in enumerate(seconds):
        B[4 * b:4 * b + 4, 4 * k:4 * k + 4] = np.eye(4)
    X, Xs = cov.solve_many(L, B), cov.solve_many(L, B, sum_panel_products_first=True)
    np.testing.assert_allclose(Xs, X, rtol=0, atol=1e-9 * np.abs(X).max())          # the same solve to rounding ...
    rows = np.concatenate([np.arange(4 * pos[a], 4 * pos[a] + 4) for a, b in pairs if pos[a] >= 0 and pos[b] >= 0])
    assert not np.array_equal(X[rows], Xs[rows])                                     # ... other bits in the rows delivered
    transposed = cov.covariance_blocks(Hs, 80, g["constant"], pairs, serve_transposed=True)
    damped = cov.covariance_blocks(Hs, 80, g["constant"], pairs, damping=1e-4)
    np.testing.assert_allclose(transposed, right, rtol=0, atol=1e-9 * np.abs(right).max())
    assert not np.array_equal(transposed, right) and not np.array_equal(damped, right)
    assert np.array_equal(transposed[-1], right[-1])                                 # (the constant pair stays zeros)
