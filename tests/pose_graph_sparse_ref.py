"""Sequential restatement of the tile-sparse pose-graph solver (include/voxgraph_amd.h, "Pose graph: the tile-sparse
solver"): the block graph's RCM order, the tiles of H, the symbolic fill of L at tile granularity, and the
factorisation, substitutions and H step that skip what is not stored -- tests/pose_graph_ref.py's per-k statements
applied tile by tile (numpy rounds the product and the difference of `T -= outer(...)` separately; nothing is summed
over k).  Matrices are dicts {(I, J): [64][64] array}, so that a graph past the dense limit fits.  Test infrastructure:
not part of the product."""
import math
import time

import numpy as np

from tests import pose_graph_ref as ref

TILE, NODES_PER_TILE = 64, 16
NATURAL, RCM, GIVEN = 0, 1, 2


# ---- order and pattern ----------------------------------------------------------------------------------------------
def rcm_order(n, pairs):
    """reverse Cuthill-McKee on the block graph: components by their lowest node, each from its minimum-degree node (ties:
    the lowest index), breadth-first, new neighbours by ascending (degree, index); the whole sequence reversed"""
    adj = [set() for _ in range(n)]
    for a, b in pairs:
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    deg = [len(s) for s in adj]
    seq, visited, grouped = [], [False] * n, [False] * n
    for v in range(n):
        if grouped[v]:
            continue
        comp, grouped[v] = [v], True
        for u in comp:
            for t in sorted(adj[u]):
                if not grouped[t]:
                    grouped[t] = True
                    comp.append(t)
        start = min(comp, key=lambda u: (deg[u], u))
        head = len(seq)
        seq.append(start)
        visited[start] = True
        while head < len(seq):
            new = [t for t in adj[seq[head]] if not visited[t]]
            for t in new:
                visited[t] = True
            seq.extend(sorted(new, key=lambda t: (deg[t], t)))
            head += 1
    return seq[::-1]


def make_order(n, pairs, ordering=NATURAL, given=None):
    """position -> free node"""
    if ordering == RCM:
        return rcm_order(n, pairs)
    return list(range(n)) if ordering == NATURAL else [int(v) for v in given]


def tile_pattern(n, pairs, order):
    """-> (H's tiles, both triangles, a set of (I, J); L's tiles [(I, J)] sorted by (column, row), the fill included)"""
    position = [0] * n
    for p, node in enumerate(order):
        position[node] = p
    nT = (n + NODES_PER_TILE - 1) // NODES_PER_TILE
    cols = [{K} for K in range(nT)]
    for a, b in pairs:
        ta, tb = position[a] // NODES_PER_TILE, position[b] // NODES_PER_TILE
        cols[min(ta, tb)].add(max(ta, tb))
    h = {(I, K) for K in range(nT) for I in cols[K]} | {(K, I) for K in range(nT) for I in cols[K]}
    for K in range(nT):
        below = sorted(cols[K] - {K})
        for j, J in enumerate(below):
            cols[J].update(below[j + 1:])
    return h, [(I, K) for K in range(nT) for I in sorted(cols[K])]


def update_triples(l_tiles):
    """the trailing updates: [(K, target (I, J), (I, K), (J, K))]"""
    out = []
    for K in sorted({J for _, J in l_tiles}):
        below = [I for I, J in l_tiles if J == K and I != K]
        out += [(K, (I, J), (I, K), (J, K)) for j, J in enumerate(below) for I in below[j:]]
    return out


def launches(l_tiles):
    n_in_column = {}
    for _, J in l_tiles:
        n_in_column[J] = n_in_column.get(J, 0) + 1
    return sum(3 if c > 1 else 1 for c in n_in_column.values())


# ---- tiles <-> dense ------------------------------------------------------------------------------------------------
def to_tiles(A, keys):
    n = A.shape[0]
    tiles = {}
    for I, J in keys:
        T = np.zeros((TILE, TILE))
        blk = A[TILE * I:min(n, TILE * I + TILE), TILE * J:min(n, TILE * J + TILE)]
        T[:blk.shape[0], :blk.shape[1]] = blk
        tiles[(I, J)] = T
    return tiles


def to_dense(tiles, n):
    A = np.zeros((n, n))
    for (I, J), T in tiles.items():
        r, c = min(TILE, n - TILE * I), min(TILE, n - TILE * J)
        A[TILE * I:TILE * I + r, TILE * J:TILE * J + c] = T[:r, :c]
    return A


def columns_of(l_tiles):
    cols = {}
    for I, J in l_tiles:
        cols.setdefault(J, []).append(I)
    return cols


# ---- the numbers ----------------------------------------------------------------------------------------------------
def cholesky(tiles, n, l_tiles):
    """in place over the L tiles (a fill tile must be there, zeros): pose_graph_ref.cholesky's statements per k -- the sqrt,
    the division of column k, the outer-product subtraction -- over the stored tiles of column k's panel alone"""
    cols = columns_of(l_tiles)
    for K in sorted(cols):
        below = [I for I in cols[K] if I != K]
        D, w = tiles[(K, K)], min(TILE, n - TILE * K)
        P = [tiles[(I, K)] for I in below]
        targets = [(tiles[(I, J)], P[i], P[j]) for j, J in enumerate(below) for i, I in enumerate(below) if i >= j]
        for k in range(w):
            akk = D[k, k]
            if not (akk > 0.0) or math.isinf(akk):
                raise ref.NotPositiveDefinite(TILE * K + k)
            D[k, k] = math.sqrt(akk)
            D[k + 1:w, k] = D[k + 1:w, k] / D[k, k]
            D[k + 1:w, k + 1:w] -= np.outer(D[k + 1:w, k], D[k + 1:w, k])
            for T in P:
                T[:, k] = T[:, k] / D[k, k]
                T[:, k + 1:] -= np.outer(T[:, k], D[k + 1:, k])
            for T, Pi, Pj in targets:
                T -= np.outer(Pi[:, k], Pj[:, k])
        D[np.triu_indices(TILE, 1)] = 0.0
    return tiles


def forward(tiles, n, l_tiles, b):
    y = np.array(b, np.float64)
    cols = columns_of(l_tiles)
    for K in sorted(cols):
        D, w, k0 = tiles[(K, K)], min(TILE, n - TILE * K), TILE * K
        below = [(TILE * I, min(TILE, n - TILE * I), tiles[(I, K)]) for I in cols[K] if I != K]
        for k in range(w):
            y[k0 + k] = y[k0 + k] / D[k, k]
            y[k0 + k + 1:k0 + w] -= D[k + 1:w, k] * y[k0 + k]
            for i0, r, T in below:
                y[i0:i0 + r] -= T[:r, k] * y[k0 + k]
    return y


def backward(tiles, n, l_tiles, y):
    x = np.array(y, np.float64)
    rows = {}
    for I, J in l_tiles:
        rows.setdefault(I, []).append(J)
    for K in sorted(rows, reverse=True):
        D, w, k0 = tiles[(K, K)], min(TILE, n - TILE * K), TILE * K
        left = [(TILE * J, tiles[(K, J)]) for J in rows[K] if J != K]
        for k in reversed(range(w)):
            x[k0 + k] = x[k0 + k] / D[k, k]
            x[k0:k0 + k] -= D[k, :k] * x[k0 + k]
            for j0, T in left:
                x[j0:j0 + TILE] -= T[k, :] * x[k0 + k]
    return x


def spd_solve(tiles, n, l_tiles, b):
    L = cholesky({key: tiles[key].copy() if key in tiles else np.zeros((TILE, TILE)) for key in l_tiles}, n, l_tiles)
    return backward(L, n, l_tiles, forward(L, n, l_tiles, b)), L


def matvec(h_tiles, n, s):
    """per row, ascending columns over the row's stored tiles, from 0.0"""
    acc = np.zeros(n)
    for I, J in sorted(h_tiles):
        T, r = h_tiles[(I, J)], min(TILE, n - TILE * I)
        for c in range(min(TILE, n - TILE * J)):
            acc[TILE * I:TILE * I + r] = acc[TILE * I:TILE * I + r] + T[:r, c] * s[TILE * J + c]
    return acc


# ---- the solve (edges only) -----------------------------------------------------------------------------------------
def joined_free_pairs(pos, reg_pairs, edges):
    """the free-node pairs of the block graph: the registration constraints, then the edges"""
    joined = [(int(a), int(b)) for a, b in reg_pairs] + [(e[0], e[1]) for e in edges]
    return [(pos[a], pos[b]) for a, b in joined if pos[a] >= 0 and pos[b] >= 0]


def assemble(n_nodes, constant, edges, terms, order, reg_pairs=(), fused=None):
    """-> (H's tiles of P H P^T, g in ascending node order, H's key set, L's tile list): every 4x4 block 0.0 plus its
    contributions in the contract's order (the fused buffer's diagonal blocks and gradients per node, its off-diagonal
    blocks per constraint (a, b) and (b, a)^T, where there are registration constraints; then the edges in list order:
    aa, bb, ab, ab^T)"""
    pos, nfree = ref.free_positions(n_nodes, constant)
    position = [0] * nfree
    for p, node in enumerate(order):
        position[node] = p
    pairs = joined_free_pairs(pos, reg_pairs, edges)
    h_keys, l_tiles = tile_pattern(nfree, pairs, order)
    H = {key: np.zeros((TILE, TILE)) for key in h_keys}
    g = np.zeros(4 * nfree)

    def add(a, b, block):
        if pos[a] >= 0 and pos[b] >= 0:
            r, c = 4 * position[pos[a]], 4 * position[pos[b]]
            H[(r // TILE, c // TILE)][r % TILE:r % TILE + 4, c % TILE:c % TILE + 4] += block

    if fused is not None:
        n = n_nodes
        diag = np.asarray(fused[1 + 4 * n:1 + 20 * n]).reshape(n, 4, 4)
        for i in range(n):
            add(i, i, diag[i])
            if pos[i] >= 0:
                g[4 * pos[i]:4 * pos[i] + 4] += fused[1 + 4 * i:5 + 4 * i]
        off = np.asarray(fused[1 + 20 * n:1 + 20 * n + 16 * len(reg_pairs)]).reshape(-1, 4, 4)
        for c, (a, b) in enumerate(reg_pairs):
            add(a, b, off[c])
            add(b, a, off[c].T)
    for e, t in zip(edges, terms):
        a, b = e[0], e[1]
        _, ga, gb, aa, bb, ab = t
        add(a, a, np.array(aa))
        add(b, b, np.array(bb))
        add(a, b, np.array(ab))
        add(b, a, np.array(ab).T)
        if pos[a] >= 0:
            g[4 * pos[a]:4 * pos[a] + 4] += np.array(ga)
        if pos[b] >= 0:
            g[4 * pos[b]:4 * pos[b] + 4] += np.array(gb)
    return H, g, h_keys, l_tiles


def permuted(v, order):
    """a vector in ascending node order -> in the order in use"""
    return np.asarray(v).reshape(-1, 4)[np.asarray(order)].ravel()


def unpermuted(v, order):
    out = np.zeros(len(v)).reshape(-1, 4)
    out[np.asarray(order)] = np.asarray(v).reshape(-1, 4)
    return out.ravel()


def solve(n_nodes, constant, edges, poses0, ordering=NATURAL, given=None, parameter_tolerance=3e-3, function_tolerance=1e-6,
          gradient_tolerance=1e-10, max_num_iterations=50, max_solver_time_in_seconds=4.0, initial_trust_region_radius=1e4,
          keep=None, registration=None):
    """pose_graph_ref.solve's loop over the tiles of P H P^T -> (poses, summary dict, history).  keep: a dict that receives
    the order, the tile lists and the last H and g.  registration: what pose_graph_ref.solve takes (None: edges only)"""
    registration = ref.ZeroRegistration() if registration is None else registration
    t0 = time.perf_counter()
    pos, nfree = ref.free_positions(n_nodes, constant)
    free_vars = [4 * i + k for i in range(n_nodes) if pos[i] >= 0 for k in range(4)]
    nf = 4 * nfree
    pairs = joined_free_pairs(pos, registration.pairs, edges)
    order = make_order(nfree, pairs, ordering, given)
    x = np.array(poses0, np.float64).reshape(n_nodes, 4).copy()
    history = []

    def total(costs, ecost):
        reg = 0.0
        for c in costs:
            reg = reg + float(c)
        return 0.5 * (reg + ecost)

    def full(p):
        fused, costs = registration.full(p)
        terms = [ref.edge_terms(e, p[e[0]], p[e[1]]) for e in edges]
        ecost = 0.0
        for t in terms:
            ecost = ecost + t[0]
        return (total(costs, ecost),) + assemble(n_nodes, constant, edges, terms, order, registration.pairs, fused)

    def cost_only(p):
        costs = registration.cost(p)
        ecost = 0.0
        for e in edges:
            ecost = ecost + ref.edge_terms(e, p[e[0]], p[e[1]], want_terms=False)
        return total(costs, ecost)

    cost, H, g, h_keys, l_tiles = full(x)
    if keep is not None:
        keep.update(order=order, h_keys=h_keys, l_tiles=l_tiles)
    initial = cost
    radius, decrease = float(initial_trust_region_radius), 2.0
    it, reason = 0, "max_iterations"
    while it < max_num_iterations:
        it += 1
        rec = dict(cost=cost, trial_cost=0.0, gain_ratio=0.0, radius=radius, step_norm=0.0, accepted=0, factorization_failed=0)
        history.append(rec)
        if np.abs(g).max() <= gradient_tolerance:
            reason = "gradient_tolerance"
            break
        A = {key: H[key].copy() if key in H else np.zeros((TILE, TILE)) for key in l_tiles}
        for K in range((nf + TILE - 1) // TILE):
            d = np.diag(H[(K, K)])[:min(TILE, nf - TILE * K)]
            idx = np.arange(len(d))
            A[(K, K)][idx, idx] = d + np.clip(d, 1e-6, 1e32) / radius
        try:
            z, _ = spd_solve(A, nf, l_tiles, permuted(g, order))
        except ref.NotPositiveDefinite:
            rec["factorization_failed"] = 1
            radius /= decrease
            decrease *= 2.0
            continue
        step_p = -z
        step, Hs = unpermuted(step_p, order), unpermuted(matvec(H, nf, step_p), order)
        xf = x.ravel()[free_vars]
        step_norm = math.sqrt(ref.dot(step, step))
        rec["step_norm"] = step_norm
        if step_norm <= parameter_tolerance * (math.sqrt(ref.dot(xf, xf)) + parameter_tolerance):
            reason = "parameter_tolerance"
            break
        cand = x.copy().ravel()
        cand[free_vars] = cand[free_vars] + step
        cand = cand.reshape(-1, 4)
        for k in range(n_nodes):
            cand[k, 3] = ref.normalize_angle(float(cand[k, 3]))
        trial = cost_only(cand)
        model_decrease = -(ref.dot(g, step) + 0.5 * ref.dot(step, Hs))
        rho = (cost - trial) / model_decrease if model_decrease > 0.0 else -1.0
        rec["trial_cost"], rec["gain_ratio"] = trial, rho
        if rho > 1e-3:
            rec["accepted"] = 1
            new_cost, H, g, _, _ = full(cand)
            rel = abs(cost - new_cost) / max(cost, 1e-300)
            x, cost = cand, new_cost
            q = 2.0 * rho - 1.0
            radius = min(radius / max(1.0 / 3.0, 1.0 - q * q * q), 1e16)
            decrease = 2.0
            if rel <= function_tolerance:
                reason = "function_tolerance"
                break
        else:
            radius /= decrease
            decrease *= 2.0
        if time.perf_counter() - t0 > max_solver_time_in_seconds:
            reason = "max_solver_time"
            break
    if keep is not None:
        keep.update(H=H, g=g)
    return x, dict(termination=reason, num_iterations=it, initial_cost=initial, final_cost=cost), history


# ---- scenes ---------------------------------------------------------------------------------------------------------
def chain_pairs(n, second=True, closures=()):
    """block pairs (i, j), i > j: a chain, its second neighbours, loop closures"""
    pairs = [(i + 1, i) for i in range(n - 1)]
    if second:
        pairs += [(i + 2, i) for i in range(n - 2)]
    return pairs + [(max(a, b), min(a, b)) for a, b in closures]


def block_matrix(n_block_rows, pairs, seed=0):
    """a symmetric positive definite matrix of 4x4 blocks: the off-diagonal blocks of `pairs` (i > j, no repeats) uniform
    in [-1, 1], each diagonal block a symmetric one plus 4 (neighbours + 1) on its diagonal (strictly diagonally dominant)
    -> dict(n, bi, bj, values [nnz][4][4] of the lower triangle, diagonal blocks first, A dense, b)"""
    rng = np.random.default_rng(seed)
    pairs = sorted(set((int(i), int(j)) for i, j in pairs))
    assert all(n_block_rows > i > j >= 0 for i, j in pairs)
    deg = np.zeros(n_block_rows, int)
    for i, j in pairs:
        deg[i] += 1
        deg[j] += 1
    n = 4 * n_block_rows
    A = np.zeros((n, n))
    bi, bj, values = [], [], []
    for i in range(n_block_rows):
        S = rng.uniform(-1, 1, (4, 4))
        S = 0.5 * (S + S.T) + 4.0 * (deg[i] + 1) * np.eye(4)
        A[4 * i:4 * i + 4, 4 * i:4 * i + 4] = S
        bi.append(i), bj.append(i), values.append(S)
    for i, j in pairs:
        B = rng.uniform(-1, 1, (4, 4))
        A[4 * i:4 * i + 4, 4 * j:4 * j + 4] = B
        A[4 * j:4 * j + 4, 4 * i:4 * i + 4] = B.T
        bi.append(i), bj.append(j), values.append(B)
    return dict(n=n, n_block_rows=n_block_rows, bi=np.array(bi, np.int32), bj=np.array(bj, np.int32), values=np.array(values), A=A,
                b=rng.uniform(-1, 1, n), pairs=pairs)


def long_graph(n=4200, seed=0, n_closures=6):
    """-> dict like pose_graph_ref.mixed_graph's, edges only: a path of n nodes winding outwards, node 0 constant;
    odometry edges k -> k + 1, second-neighbour edges k -> k + 2, n_closures loop closures between far nodes; every
    observation the true relative pose plus seeded noise, the start poses the true ones plus seeded noise"""
    rng = np.random.default_rng(seed)
    s = np.arange(n) * 0.05
    true = np.stack([(1.0 + 0.2 * s) * np.cos(s), (1.0 + 0.2 * s) * np.sin(s), 0.01 * s, 0.3 * np.sin(0.7 * s)], 1)
    true -= true[0]

    def noisy(a, b, information_diag):
        _, _, t, yaw, S = ref.relative_edge(a, b, true[a], true[b], information_diag)
        return (int(a), int(b), [v + rng.normal(0, 0.01) for v in t], ref.normalize_angle(yaw + rng.normal(0, 0.002)), S)

    edges = [noisy(k, k + 1, ref.INFO_ODOMETRY) for k in range(n - 1)]
    edges += [noisy(k, k + 2, ref.INFO_ODOMETRY) for k in range(n - 2)]
    far = np.linspace(0, n - 1, 2 * n_closures + 2).astype(int)[1:-1]
    edges += [noisy(int(far[-1 - i]), int(far[i]), ref.INFO_LOOP_CLOSURE) for i in range(n_closures)]
    constant = [1] + [0] * (n - 1)
    poses0 = true + rng.normal(0, 1, (n, 4)) * np.array([0.05, 0.05, 0.02, 0.01])
    poses0[0] = true[0]
    return dict(n=n, true=true, poses0=poses0, pairs=[], edges=edges, constant=constant)
