"""Sequential restatement of the pose-graph solve (include/voxgraph_amd.h, "Pose graph: the solve"): the
order contract written out, one rounded operation at a time, so that the library can be compared with it bit for bit.

Edge terms are Python floats through math.sin / math.cos (the libm the library's host code calls); the assembly is a
loop over contributions in the contract's order; the Cholesky factorisation is the unblocked right-looking one (numpy
rounds the product and the difference of `A -= outer(...)` separately); the substitutions are column-oriented; every
dot product and norm is an ascending loop from 0.0.  Test infrastructure: not part of the product."""
import math
import time

import numpy as np

TWO_PI = 2.0 * math.pi
REASONS = ("parameter_tolerance", "function_tolerance", "gradient_tolerance", "max_iterations", "max_solver_time",
           "no_free_nodes")


class NotPositiveDefinite(Exception):
    pass


def normalize_angle(a):
    return a - TWO_PI * math.floor((a + math.pi) / TWO_PI)


def edge_terms(edge, pa, pb, want_terms=True):
    """edge = (a, b, t_obs[3], yaw_obs, S[4][4]) -> cost, or (cost, ga[4], gb[4], aa, bb, ab [4][4] lists)"""
    _, _, t_obs, yaw_obs, S = edge
    pa, pb = [float(v) for v in pa], [float(v) for v in pb]
    t_obs, S = [float(v) for v in t_obs], [[float(v) for v in row] for row in np.asarray(S).reshape(4, 4)]
    c, s = math.cos(pa[3]), math.sin(pa[3])
    d0, d1, d2 = pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]
    err = [c * d0 + s * d1 - t_obs[0], -s * d0 + c * d1 - t_obs[1], d2 - t_obs[2],
           normalize_angle(pb[3] - pa[3] - float(yaw_obs))]
    r = []
    for i in range(4):
        acc = 0.0
        for k in range(4):
            acc = acc + S[i][k] * err[k]
        r.append(acc)
    cost = 0.0
    for i in range(4):
        cost = cost + r[i] * r[i]
    if not want_terms:
        return cost
    Jb = [[0.0] * 4 for _ in range(4)]
    Jb[0][0], Jb[0][1], Jb[1][0], Jb[1][1], Jb[2][2], Jb[3][3] = c, s, -s, c, 1.0, 1.0
    Ja = [[-v for v in row] for row in Jb]
    Ja[0][3] = -s * d0 + c * d1
    Ja[1][3] = -c * d0 - s * d1

    def left(J):
        out = [[0.0] * 4 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                acc = 0.0
                for k in range(4):
                    acc = acc + S[i][k] * J[k][j]
                out[i][j] = acc
        return out

    def jtr(J):
        out = []
        for i in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + J[k][i] * r[k]
            out.append(acc)
        return out

    def jtj(P, Q):
        out = [[0.0] * 4 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                acc = 0.0
                for k in range(4):
                    acc = acc + P[k][i] * Q[k][j]
                out[i][j] = acc
        return out

    SJa, SJb = left(Ja), left(Jb)
    return cost, jtr(SJa), jtr(SJb), jtj(SJa, SJa), jtj(SJb, SJb), jtj(SJa, SJb)


def free_positions(n_nodes, constant):
    pos, k = [], 0
    for i in range(n_nodes):
        if constant[i]:
            pos.append(-1)
        else:
            pos.append(k)
            k += 1
    return pos, k


def assemble(n_nodes, constant, pairs, fused, edges, terms, swap_steps_2_and_3=False, drop_transpose=False):
    """The reduced H [4f][4f] and g [4f]: every block 0.0 plus its contributions in the contract's order.  fused: the
    buffer of vgx_reg_batch_assemble, or None (registration excluded); terms[e] = edge_terms(edges[e], ...).  The two
    flags build the WRONG system of the mutation checks (tests/test_pose_graph_gpu.py)."""
    pos, nfree = free_positions(n_nodes, constant)
    H, g = np.zeros((4 * nfree, 4 * nfree)), np.zeros(4 * nfree)

    def add(a, b, block):
        if pos[a] >= 0 and pos[b] >= 0:
            H[4 * pos[a]:4 * pos[a] + 4, 4 * pos[b]:4 * pos[b] + 4] += block

    def step_1_and_2(only=None):
        if fused is None:
            return
        n = n_nodes
        if only in (None, 1):
            diag = np.asarray(fused[1 + 4 * n:1 + 20 * n]).reshape(n, 4, 4)
            for i in range(n):
                add(i, i, diag[i])
                if pos[i] >= 0:
                    g[4 * pos[i]:4 * pos[i] + 4] += fused[1 + 4 * i:5 + 4 * i]
        if only in (None, 2):
            off = np.asarray(fused[1 + 20 * n:1 + 20 * n + 16 * len(pairs)]).reshape(-1, 4, 4)
            for c, (a, b) in enumerate(pairs):
                add(a, b, off[c])
                if not drop_transpose:
                    add(b, a, off[c].T)

    def step_3():
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

    if swap_steps_2_and_3:
        step_1_and_2(only=1)
        step_3()
        step_1_and_2(only=2)
    else:
        step_1_and_2()
        step_3()
    return H, g


_CHOLESKY_STRIP = 64


def cholesky(A, sum_products_first=False):
    """Unblocked right-looking Cholesky of the lower triangle of A -> L (zeros above the diagonal)."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    if sum_products_first:                     # the WRONG order of the mutation check: per 64-wide panel, products summed first
        return _cholesky_summed(A)
    # `A[k + 1:, k + 1:] -= outer(column k, column k)` for k ascending, in an order of loops that keeps a strip of columns in
    # the cache: a strip first takes the products of every finished column left of it, k ascending, then its own columns'
    # as they are finished.  Every element below the diagonal sees the statement's operations in the statement's order --
    # per k one rounded product, then one rounded difference -- and a bad pivot is still the first in ascending k; what the
    # strips skip lies above the diagonal and is dropped at the end.
    products = np.empty((n, min(n, _CHOLESKY_STRIP)))
    for c0 in range(0, n, _CHOLESKY_STRIP):
        c1 = min(n, c0 + _CHOLESKY_STRIP)
        strip, p = A[c0:, c0:c1], products[:n - c0, :c1 - c0]
        for k in range(c0):
            np.multiply(A[c0:, k, None], A[None, c0:c1, k], out=p)
            np.subtract(strip, p, out=strip)
        for k in range(c0, c1):
            akk = A[k, k]
            if not (akk > 0.0) or math.isinf(akk):
                raise NotPositiveDefinite(k)
            A[k, k] = math.sqrt(akk)
            A[k + 1:, k] = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:c1] -= np.outer(A[k + 1:, k], A[k + 1:c1, k])
    return np.tril(A)


def _cholesky_summed(A):
    n = A.shape[0]
    for k0 in range(0, n, 64):
        w = min(64, n - k0)
        A[k0:k0 + w, k0:k0 + w] = cholesky(np.tril(A[k0:k0 + w, k0:k0 + w]) + np.tril(A[k0:k0 + w, k0:k0 + w], -1).T)
        L11 = A[k0:k0 + w, k0:k0 + w]
        for j in range(w):
            A[k0 + w:, k0 + j] = A[k0 + w:, k0 + j] / L11[j, j]
            A[k0 + w:, k0 + j + 1:k0 + w] -= np.outer(A[k0 + w:, k0 + j], L11[j + 1:, j])
        P = A[k0 + w:, k0:k0 + w]
        A[k0 + w:, k0 + w:] -= P @ P.T
    return np.tril(A)


def forward(L, b):
    y = np.array(b, np.float64)
    n = len(y)
    for j in range(n):
        y[j] = y[j] / L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    return y


def backward(L, y):
    x = np.array(y, np.float64)
    n = len(x)
    for j in reversed(range(n)):
        x[j] = x[j] / L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


def spd_solve(A, b, **kw):
    L = cholesky(A, **kw)
    return backward(L, forward(L, b)), L


def matvec(H, s):
    acc = np.zeros(H.shape[0])
    for c in range(H.shape[1]):
        acc = acc + H[:, c] * s[c]
    return acc


def dot(a, b):
    acc = 0.0
    for x, y in zip(a, b):
        acc = acc + float(x) * float(y)
    return acc


class ZeroRegistration:
    """no registration constraints (or excluded ones)"""
    pairs = ()

    def full(self, poses):
        return None, ()

    def cost(self, poses):
        return ()


class BackendRegistration:
    """a harness backend (poses -> fused buffer): buffer[0] is the list-order sum of the per-constraint costs already"""

    def __init__(self, backend, pairs):
        self.backend, self.pairs = backend, [(int(a), int(b)) for a, b in pairs]

    def full(self, poses):
        buf = np.array(self.backend(poses))
        return buf, (buf[0],)

    def cost(self, poses):
        return (np.asarray(self.backend(poses))[0],)


def solve(registration, n_nodes, constant, edges, poses0, parameter_tolerance=3e-3, function_tolerance=1e-6,
          gradient_tolerance=1e-10, max_num_iterations=50, max_solver_time_in_seconds=4.0, initial_trust_region_radius=1e4):
    """-> (poses, summary dict, history list of dicts): the loop of the header, restated."""
    t0 = time.perf_counter()
    pos, nfree = free_positions(n_nodes, constant)
    free_vars = [4 * i + k for i in range(n_nodes) if pos[i] >= 0 for k in range(4)]
    nf = 4 * nfree
    x = np.array(poses0, np.float64).reshape(n_nodes, 4).copy()
    history = []
    if nf == 0:
        return x, dict(termination="no_free_nodes", num_iterations=0, initial_cost=0.0, final_cost=0.0), history

    def total(costs, ecost):
        reg = 0.0
        for c in costs:
            reg = reg + float(c)
        return 0.5 * (reg + ecost)

    def full(p):
        fused, costs = registration.full(p)
        terms = [edge_terms(e, p[e[0]], p[e[1]]) for e in edges]
        ecost = 0.0
        for t in terms:
            ecost = ecost + t[0]
        H, g = assemble(n_nodes, constant, registration.pairs, fused, edges, terms)
        return total(costs, ecost), g, H

    def cost_only(p):
        costs = registration.cost(p)
        ecost = 0.0
        for e in edges:
            ecost = ecost + edge_terms(e, p[e[0]], p[e[1]], want_terms=False)
        return total(costs, ecost)

    cost, g, H = full(x)
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
        d2 = np.clip(np.diag(H), 1e-6, 1e32)
        A = H.copy()
        A[np.arange(nf), np.arange(nf)] = np.diag(H) + d2 / radius
        try:
            z, _ = spd_solve(A, g)
        except NotPositiveDefinite:
            rec["factorization_failed"] = 1
            radius /= decrease
            decrease *= 2.0
            continue
        step = -z
        Hs = matvec(H, step)
        xf = x.ravel()[free_vars]
        step_norm = math.sqrt(dot(step, step))
        rec["step_norm"] = step_norm
        if step_norm <= parameter_tolerance * (math.sqrt(dot(xf, xf)) + parameter_tolerance):
            reason = "parameter_tolerance"
            break
        cand = x.copy().ravel()
        cand[free_vars] = cand[free_vars] + step
        cand = cand.reshape(-1, 4)
        for k in range(n_nodes):
            cand[k, 3] = normalize_angle(float(cand[k, 3]))
        trial = cost_only(cand)
        model_decrease = -(dot(g, step) + 0.5 * dot(step, Hs))
        rho = (cost - trial) / model_decrease if model_decrease > 0.0 else -1.0
        rec["trial_cost"], rec["gain_ratio"] = trial, rho
        if rho > 1e-3:
            rec["accepted"] = 1
            new_cost, g, H = full(cand)
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
    return x, dict(termination=reason, num_iterations=it, initial_cost=initial, final_cost=cost), history


# ---------------------------------------------------------------------------
# the graph the CPU and GPU tests share: small submaps on a ring, odometry with drift, two loop closures
# ---------------------------------------------------------------------------
INFO_ODOMETRY = (1.0, 1.0, 2500.0, 2500.0)            # voxgraph_mapper.yaml:41-47
INFO_LOOP_CLOSURE = (100.0, 100.0, 2500.0, 2500.0)


def relative_edge(a, b, pose_a, pose_b, information_diag):
    """the edge whose observation is the relative pose of pose_b in pose_a, sqrt-information diag(sqrt(information))"""
    c, s = math.cos(pose_a[3]), math.sin(pose_a[3])
    d = [float(pose_b[k] - pose_a[k]) for k in range(3)]
    t = [c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2]]
    return (int(a), int(b), t, normalize_angle(float(pose_b[3] - pose_a[3])), np.diag(np.sqrt(np.asarray(information_diag, np.float64))))


def ring_graph(n=12, seed=0, drift=(0.03, -0.02, 0.0, 0.008), block_dims=(2, 2, 2)):
    """-> dict: true poses, start poses (odometry with an accumulating bias plus seeded noise), registration pairs
    (consecutive nodes), edges (n - 1 odometry edges, loop closures n-1 -> 0 and 2n/3 -> n/6), the scene's sdf."""
    from oracle import synth
    sdf = synth.union_sdf(synth.sphere_ground_sdf((1.6, 1.6, 1.2), 1.0, 0.35), synth.sphere_sdf((0.6, 2.4, 0.8), 0.5))
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    true = np.stack([0.5 * np.cos(ang) - 0.5, 0.5 * np.sin(ang), 0.01 * np.arange(n), 0.1 * np.sin(ang)], 1)
    true[0] = 0
    rng = np.random.default_rng(seed)
    poses0 = true.copy()
    for k in range(1, n):
        poses0[k] = poses0[k - 1] + (true[k] - true[k - 1]) + np.asarray(drift) + rng.normal(0, 0.004, 4)
    pairs = [(k, k + 1) for k in range(n - 1)]
    edges = [relative_edge(k, k + 1, poses0[k], poses0[k + 1], INFO_ODOMETRY) for k in range(n - 1)]
    edges.append(relative_edge(n - 1, 0, true[n - 1], true[0], INFO_LOOP_CLOSURE))
    edges.append(relative_edge(2 * n // 3, n // 6, true[2 * n // 3], true[n // 6], INFO_LOOP_CLOSURE))
    constant = [1] + [0] * (n - 1)
    return dict(n=n, sdf=sdf, true=true, poses0=poses0, pairs=pairs, edges=edges, constant=constant, block_dims=block_dims)


def ring_submaps(graph, voxel_size=0.1, vps=16):
    from oracle import synth
    return [synth.make_submap(graph["sdf"], voxel_size, vps, (0, 0, 0), graph["block_dims"], 0.3, p, 1.0, drop_empty_blocks=True)
            for p in graph["true"]]


def mixed_graph(n=80, seed=0):
    """-> dict like ring_graph's, edges only (pairs = []): the node-to-free-position map, long contribution lists and
    the yaw wrap at work.  Constant nodes 0, n // 3 and 2 n // 3 + 1, so a free node's position is i - 1, i - 2 or
    i - 3.  Nodes on a circle of 3 m radius, the true yaws once around the full circle and half again.  Edges, in list
    order: the chain k -> k + 1 (diagonal sqrt-information; two of them start at a constant node, two end at one); the
    hub, node 5, joined to 32 nodes spread over the list, alternately as `a` and as `b`, each with a full non-symmetric
    sqrt-information; the chain's pair (10, 11) once more in the opposite direction, 11 -> 10, full as well; one edge
    from the constant node n // 3 to the hub.  Every observation is the true relative pose plus seeded noise, so the
    optimum keeps a cost and the gain ratios are not 1.  The yaw information (1) is small next to the translation's, so
    the yaws follow from R(yaw_a)^T (t_b - t_a) -- the nonlinear part -- and a Gauss-Newton step from a start a metre
    and a radian off can be rejected.  The start poses are the true ones plus seeded noise, every yaw then shifted by
    a random multiple of 2 pi in [-2, 2]: they arrive unwrapped."""
    assert n >= 40
    translation_noise, yaw_noise = 0.05, 0.05            # of the observations: metres, radians
    start_noise = (1.0, 1.0, 0.1, 1.0)                   # of the start poses: x y z yaw
    yaw_information = 1.0
    odometry, closure = INFO_ODOMETRY[:3] + (yaw_information,), INFO_LOOP_CLOSURE[:3] + (yaw_information,)
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    true = np.stack([3.0 * np.cos(ang) - 3.0, 3.0 * np.sin(ang), 0.02 * np.arange(n), 1.5 * ang], 1)
    true[:, 3] = [normalize_angle(float(v)) for v in true[:, 3]]
    constant = [0] * n
    for k in (0, n // 3, 2 * n // 3 + 1):
        constant[k] = 1
    hub = 5

    def noisy(a, b, information_diag, full):
        _, _, t, yaw, S = relative_edge(a, b, true[a], true[b], information_diag)
        t = [v + rng.normal(0, translation_noise) for v in t]
        yaw = normalize_angle(yaw + rng.normal(0, yaw_noise))
        if full:
            S = S + rng.normal(0, 2.0, (4, 4))
        return (int(a), int(b), t, yaw, S)

    edges = [noisy(k, k + 1, odometry, False) for k in range(n - 1)]
    others = [k for k in range(n) if k != hub and k != n // 3][1::2][:32]
    for i, k in enumerate(others):
        edges.append(noisy(hub, k, closure, True) if i % 2 == 0 else noisy(k, hub, closure, True))
    edges.append(noisy(11, 10, closure, True))
    edges.append(noisy(n // 3, hub, closure, True))
    free = 1.0 - np.asarray(constant, np.float64)[:, None]
    poses0 = true + free * rng.normal(0, 1, (n, 4)) * np.asarray(start_noise)
    poses0[:, 3] += TWO_PI * rng.integers(-2, 3, n)
    return dict(n=n, true=true, poses0=poses0, pairs=[], edges=edges, constant=constant, hub=hub)


MIXED_SEED = 12          # pinned on the CPU: with it the restatement's solve of mixed_graph(80) accepts, rejects and wraps
MIXED_SOLVE = dict(parameter_tolerance=1e-6, function_tolerance=1e-8, max_num_iterations=30, initial_trust_region_radius=1e4)
# the assembly scene: mixed_graph(80)'s edges plus six registration constraints among the six submaps of ring_graph(6),
# submap k standing at node ASSEMBLY_NODES[k] -- a constant node, the hub, and the pair (10, 11), which then carries a
# chain edge, the edge 11 -> 10 and a registration constraint in either direction
ASSEMBLY_NODES = (26, 10, 11, 5, 40, 79)
ASSEMBLY_SUBMAP_PAIRS = ((1, 2), (2, 1), (0, 3), (3, 4), (4, 5), (2, 5))


def assembly_scene():
    """-> (mixed graph, ring_graph(6), registration pairs in node indices, poses [80][4]: the mixed graph's start poses,
    the six nodes with a submap at the ring's start poses so that the submaps overlap as they do there)"""
    g, ring = mixed_graph(80, MIXED_SEED), ring_graph(6, seed=0)
    pairs = [(ASSEMBLY_NODES[a], ASSEMBLY_NODES[b]) for a, b in ASSEMBLY_SUBMAP_PAIRS]
    poses = g["poses0"].copy()
    for k, node in enumerate(ASSEMBLY_NODES):
        poses[node] = ring["poses0"][k]
    return g, ring, pairs, poses


def touched_blocks(n_nodes, constant, pairs, edges):
    """[f][f] bool: the 4x4 blocks of the reduced H that some constraint contributes to"""
    pos, nfree = free_positions(n_nodes, constant)
    touched = np.zeros((nfree, nfree), bool)
    for a, b in list(pairs) + [(e[0], e[1]) for e in edges]:
        for i, j in ((a, a), (b, b), (a, b), (b, a)):
            if pos[i] >= 0 and pos[j] >= 0:
                touched[pos[i], pos[j]] = True
    return touched


def unwrapped_yaw_errors(graph, poses):
    """yaw_b - yaw_a - yaw_obs of every edge BEFORE the wrap"""
    return np.array([float(poses[b][3]) - float(poses[a][3]) - float(yaw) for a, b, _, yaw, _ in graph["edges"]])


def lm_edges(edges):
    """the same edges for harness/lm.py (diagonal information only)"""
    from harness import lm
    return [lm.RelativePoseEdge(a, b, t, yaw, np.diag(S) ** 2) for a, b, t, yaw, S in edges]
