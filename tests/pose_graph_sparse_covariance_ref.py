"""Sequential restatement of the edge covariances on the tile-sparse factor (include/voxgraph_amd.h, "Pose graph: edge
covariances on the tile-sparse factor"): tests/pose_graph_sparse_ref.py's cholesky, and its forward / backward with an
[n][m] right-hand side -- np.outer, then the subtraction, so every element keeps the one rounded multiply and one rounded
subtract per k that forward / backward give its column.  Then the column list, the positions under the order in use,
the slabs and the block extraction.  Nothing is skipped here: the skips of the kernel change no delivered bit, which is
what the GPU tests check against this.  numpy only.  Test infrastructure: not part of the product."""
import numpy as np

from tests import pose_graph_ref as ref
from tests import pose_graph_sparse_ref as sref
from tests.pose_graph_ref import NotPositiveDefinite  # noqa: F401  (what covariance_blocks raises)

TILE = sref.TILE
CHUNK = 32                   # columns one workgroup owns
DEFAULT_BUDGET = 1 << 30     # max_solve_bytes == 0


# ---- the substitutions on many right-hand sides ---------------------------------------------------------------------
def forward_many(tiles, n, l_tiles, B):
    Y = np.array(B, np.float64)
    cols = sref.columns_of(l_tiles)
    for K in sorted(cols):
        D, w, k0 = tiles[(K, K)], min(TILE, n - TILE * K), TILE * K
        below = [(TILE * I, min(TILE, n - TILE * I), tiles[(I, K)]) for I in cols[K] if I != K]
        for k in range(w):
            Y[k0 + k] = Y[k0 + k] / D[k, k]
            Y[k0 + k + 1:k0 + w] -= np.outer(D[k + 1:w, k], Y[k0 + k])
            for i0, r, T in below:
                Y[i0:i0 + r] -= np.outer(T[:r, k], Y[k0 + k])
    return Y


def backward_many(tiles, n, l_tiles, Y):
    X = np.array(Y, np.float64)
    rows = {}
    for I, J in l_tiles:
        rows.setdefault(I, []).append(J)
    for K in sorted(rows, reverse=True):
        D, w, k0 = tiles[(K, K)], min(TILE, n - TILE * K), TILE * K
        left = [(TILE * J, tiles[(K, J)]) for J in rows[K] if J != K]
        for k in reversed(range(w)):
            X[k0 + k] = X[k0 + k] / D[k, k]
            X[k0:k0 + k] -= np.outer(D[k, :k], X[k0 + k])
            for j0, T in left:
                X[j0:j0 + TILE] -= np.outer(T[k, :], X[k0 + k])
    return X


def factor(tiles, n, l_tiles):
    """the tiles of L from the tiles of the matrix (a fill tile starts at +0.0); raises NotPositiveDefinite"""
    return sref.cholesky({key: tiles[key].copy() if key in tiles else np.zeros((TILE, TILE)) for key in l_tiles}, n, l_tiles)


def solve_many(L, n, l_tiles, B):
    """X [n][m] with L L^T X = B over the stored tiles: column c is sref.backward(sref.forward(B[:, c])) bit for bit"""
    return backward_many(L, n, l_tiles, forward_many(L, n, l_tiles, B))


# ---- columns, positions, slabs --------------------------------------------------------------------------------------
def positions(n_nodes, constant, order):
    """node -> position under the order in use (order: position -> free node), -1 for a constant node"""
    pos, nfree = ref.free_positions(n_nodes, constant)
    place = [0] * nfree
    for p, node in enumerate(order):
        place[node] = p
    return [place[pos[i]] if pos[i] >= 0 else -1 for i in range(n_nodes)]


def column_lists(place, pairs):
    """-> (second positions ascending, {position: first column}, unit rows [m], chunk rows [ceil(m / 32)][2]): per chunk of
    32 columns the row of its first column's 1 and the lowest row any pair of its columns wants"""
    seconds = sorted({place[b] for a, b in pairs if place[a] >= 0 and place[b] >= 0})
    col = {q: 4 * k for k, q in enumerate(seconds)}
    unit_rows = [4 * q + k for q in seconds for k in range(4)]
    lowest = {}
    for a, b in pairs:
        if place[a] >= 0 and place[b] >= 0:
            lowest[place[b]] = min(lowest.get(place[b], 4 * place[a]), 4 * place[a])
    chunks = []
    for c0 in range(0, len(unit_rows), CHUNK):
        nodes = [q for q in seconds if c0 <= col[q] < c0 + CHUNK]
        chunks.append((unit_rows[c0], min(lowest[q] for q in nodes)))
    return seconds, col, unit_rows, chunks


def slab_width(nf, m, max_solve_bytes=0):
    """S: the largest multiple of 32 with 8 nf S <= the budget, 32 at the least, and no more than the columns there are"""
    budget = DEFAULT_BUDGET if max_solve_bytes == 0 else max_solve_bytes
    m_round = max(CHUNK, (m + CHUNK - 1) // CHUNK * CHUNK)
    return max(CHUNK, min(m_round, budget // (8 * nf) // CHUNK * CHUNK))


def slab_pairs(place, pairs, col, S):
    """per slab the indices of the pairs (between free nodes) whose second node's columns lie in it, in list order"""
    n_slabs = (4 * len(col) + S - 1) // S
    out = [[] for _ in range(n_slabs)]
    for p, (a, b) in enumerate(pairs):
        if place[a] >= 0 and place[b] >= 0:
            out[col[place[b]] // S].append(p)
    return out


def expected_stats(nf, l_tiles, place, pairs, max_solve_bytes=0):
    _, col, unit_rows, _ = column_lists(place, pairs)
    m = len(unit_rows)
    S = slab_width(nf, m, max_solve_bytes)
    n_slabs = (m + S - 1) // S
    return dict(n_columns=m, n_slabs=n_slabs, n_launches=1 + sref.launches(l_tiles) + 4 * n_slabs,
                solve_bytes=8 * nf * min(S, m) if m else 0)


# ---- the blocks -----------------------------------------------------------------------------------------------------
def permuted_tiles(H, order, h_keys):
    """H dense in ascending node order -> the tiles `h_keys` of P H P^T"""
    P = np.repeat(4 * np.asarray(order), 4) + np.tile(np.arange(4), len(order))
    return sref.to_tiles(np.asarray(H, np.float64)[np.ix_(P, P)], sorted(h_keys))


def covariance_blocks(h_tiles, nf, l_tiles, place, pairs, L=None, want_columns=False):
    """[n_pairs][4][4]: block (a, b) = the solved columns of node b at rows 4 place[a] .. + 3 of (P H P^T)^-1, from the
    undamped tiled factor; zeros where a or b is constant.  h_tiles: the tiles of P H P^T.  L: factor(...) where the
    caller has it.  want_columns: also X [nf][m] and the column map"""
    pairs = [(int(a), int(b)) for a, b in pairs]
    out = np.zeros((len(pairs), 4, 4))
    if nf == 0:
        return out
    if L is None:
        L = factor(h_tiles, nf, l_tiles)
    seconds, col, unit_rows, _ = column_lists(place, pairs)
    X = np.zeros((nf, 0))
    if seconds:
        B = np.zeros((nf, len(unit_rows)))
        B[unit_rows, np.arange(len(unit_rows))] = 1.0
        X = solve_many(L, nf, l_tiles, B)
        for p, (a, b) in enumerate(pairs):
            if place[a] >= 0 and place[b] >= 0:
                out[p] = X[4 * place[a]:4 * place[a] + 4, col[place[b]]:col[place[b]] + 4]
    return (out, X, col) if want_columns else out


def structure(n_nodes, constant, joined, ordering=sref.NATURAL, given=None):
    """joined: the node pairs that constraints join -> (order, place, H's tile keys, L's tile list)"""
    pos, nfree = ref.free_positions(n_nodes, constant)
    free_pairs = [(pos[a], pos[b]) for a, b in joined if pos[a] >= 0 and pos[b] >= 0]
    order = sref.make_order(nfree, free_pairs, ordering, given)
    h_keys, l_tiles = sref.tile_pattern(nfree, free_pairs, order)
    return order, positions(n_nodes, constant, order), h_keys, l_tiles


def chain_with_closures(n=60, seed=5):
    """pose_graph_covariance_ref.chain_graph's shape at 60 nodes: a chain, node 0 constant, three loop closures"""
    from tests import pose_graph_covariance_ref as cov
    return cov.chain_graph(n, seed=seed)


def two_components(n=50, seed=2):
    """-> an edges-only graph dict of two disconnected components, each anchored by a constant node: nodes 0 .. n/2 - 1 a
    chain (node 0 constant), nodes n/2 .. n - 1 a chain (node n/2 constant) with a hub joined to every fourth node of it"""
    rng = np.random.default_rng(seed)
    h = n // 2
    ang = np.linspace(0, 1.2 * np.pi, n)
    true = np.stack([8.0 * np.cos(ang), 8.0 * np.sin(ang), 0.02 * np.arange(n), ang / 4.0], 1)

    def noisy(a, b, information):
        a_, b_, t, yaw, S = ref.relative_edge(a, b, true[a], true[b], information)
        return (a_, b_, [v + rng.normal(0, 0.02) for v in t], ref.normalize_angle(yaw + rng.normal(0, 0.01)), S)

    edges = [noisy(k, k + 1, ref.INFO_ODOMETRY) for k in range(n - 1) if k + 1 != h]
    hub = h + 7
    edges += [noisy(hub, k, ref.INFO_LOOP_CLOSURE) for k in range(h, n, 4) if abs(k - hub) > 1]
    constant = [1 if k in (0, h) else 0 for k in range(n)]
    poses0 = true + (1.0 - np.asarray(constant, np.float64)[:, None]) * rng.normal(0, 0.05, (n, 4))
    return dict(n=n, true=true, poses0=poses0, pairs=[], edges=edges, constant=constant, hub=hub)
