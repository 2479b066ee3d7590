"""Sequential restatement of the pose-graph edge covariances (include/voxgraph_amd.h, "Pose graph: edge covariances"):
tests/pose_graph_ref.py's cholesky / forward / backward applied to every right-hand side.  numpy only.  solve_many is
vectorised over the columns with an elementwise multiply and then an elementwise subtract, so every element keeps the
history forward / backward give its column.  Test infrastructure: not part of the product."""
import numpy as np

from tests import pose_graph_ref as ref
from tests.pose_graph_ref import NotPositiveDefinite  # noqa: F401  (what covariance_blocks raises)


def solve_many(L, B, sum_panel_products_first=False):
    """X [n][m] with L L^T X = B: column c is ref.backward(L, ref.forward(L, B[:, c])) bit for bit.  The flag builds the
    WRONG order of the mutation check: per 64-wide panel the other rows' products are summed before they are subtracted."""
    L = np.asarray(L, np.float64)
    X = np.array(B, np.float64)
    n = X.shape[0]
    if sum_panel_products_first:
        return _solve_many_summed(L, X)
    for j in range(n):
        X[j] = X[j] / L[j, j]
        X[j + 1:] -= L[j + 1:, j, None] * X[j]
    for j in reversed(range(n)):
        X[j] = X[j] / L[j, j]
        X[:j] -= L[j, :j, None] * X[j]
    return X


def _solve_many_summed(L, X):
    n = X.shape[0]
    for k0 in range(0, n, 64):
        k1 = min(k0 + 64, n)
        for j in range(k0, k1):
            X[j] = X[j] / L[j, j]
            X[j + 1:k1] -= L[j + 1:k1, j, None] * X[j]
        X[k1:] -= L[k1:, k0:k1] @ X[k0:k1]
    for k0 in reversed(range(0, n, 64)):
        k1 = min(k0 + 64, n)
        for j in reversed(range(k0, k1)):
            X[j] = X[j] / L[j, j]
            X[k0:j] -= L[j, k0:j, None] * X[j]
        X[:k0] -= L[k0:k1, :k0].T @ X[k0:k1]
    return X


def covariance_blocks(H, n_nodes, constant, pairs, damping=None, serve_transposed=False, L=None):
    """[n_pairs][4][4]: block (a, b) = the solution columns of node b of H^-1 at the rows of node a, H factorised
    undamped; zeros where a or b is constant.  Raises NotPositiveDefinite where the factorisation does.  Only the
    distinct second nodes are solved, in ascending free position (which columns are solved together changes no bit).
    The two keywords build the WRONG answers of the mutation checks: H + damping * diag(H); (a, b) served as the
    transpose of (b, a).  L: ref.cholesky(H) where the caller has it already."""
    pos, nfree = ref.free_positions(n_nodes, constant)
    H = np.asarray(H, np.float64)
    assert H.shape == (4 * nfree, 4 * nfree)
    pairs = [(int(a), int(b)) for a, b in pairs]
    if serve_transposed:
        return np.stack([blk.T for blk in covariance_blocks(H, n_nodes, constant, [(b, a) for a, b in pairs], damping)])
    out = np.zeros((len(pairs), 4, 4))
    if nfree == 0:
        return out
    if L is None:
        A = H.copy()
        if damping is not None:
            A[np.arange(4 * nfree), np.arange(4 * nfree)] = np.diag(H) + damping * np.diag(H)
        L = ref.cholesky(A)
    seconds = sorted({pos[b] for a, b in pairs if pos[a] >= 0 and pos[b] >= 0})
    if not seconds:
        return out
    B = np.zeros((4 * nfree, 4 * len(seconds)))
    for k, b in enumerate(seconds):
        B[4 * b:4 * b + 4, 4 * k:4 * k + 4] = np.eye(4)
    X = solve_many(L, B)
    col = {b: 4 * k for k, b in enumerate(seconds)}
    for p, (a, b) in enumerate(pairs):
        if pos[a] >= 0 and pos[b] >= 0:
            out[p] = X[4 * pos[a]:4 * pos[a] + 4, col[pos[b]]:col[pos[b]] + 4]
    return out


def assembled_system(g, poses=None):
    """H, g of an edges-only graph dict (ref.ring_graph / ref.mixed_graph shape) at `poses` (default: its start poses)"""
    poses = g["poses0"] if poses is None else poses
    terms = [ref.edge_terms(e, poses[e[0]], poses[e[1]]) for e in g["edges"]]
    return ref.assemble(g["n"], g["constant"], (), None, g["edges"], terms)


def chain_graph(n=300, seed=3):
    """-> dict like ref.mixed_graph's, edges only: a chain of n nodes along a slow arc, node 0 constant (nf = 4 (n - 1)),
    odometry k -> k + 1 and loop closures (n - 1 -> 0, 2n/3 -> n/6, n/2 -> n/4) with seeded observation noise"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 1.5 * np.pi, n)
    true = np.stack([20.0 * np.cos(ang) - 20.0, 20.0 * np.sin(ang), 0.01 * np.arange(n), ang / 3.0], 1)
    constant = [1] + [0] * (n - 1)

    def noisy(a, b, information):
        a_, b_, t, yaw, S = ref.relative_edge(a, b, true[a], true[b], information)
        return (a_, b_, [v + rng.normal(0, 0.02) for v in t], ref.normalize_angle(yaw + rng.normal(0, 0.01)), S)

    edges = [noisy(k, k + 1, ref.INFO_ODOMETRY) for k in range(n - 1)]
    edges += [noisy(a, b, ref.INFO_LOOP_CLOSURE) for a, b in ((n - 1, 0), (2 * n // 3, n // 6), (n // 2, n // 4))]
    poses0 = true + (1.0 - np.asarray(constant, np.float64)[:, None]) * rng.normal(0, 0.05, (n, 4))
    return dict(n=n, true=true, poses0=poses0, pairs=[], edges=edges, constant=constant)
