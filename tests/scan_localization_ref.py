"""Sequential restatement of scan localisation (include/voxgraph_amd.h, "Scan localisation"): a scan's points
against posed, finished submaps -- the formulation in numpy f32 (every numpy op rounds once, as the kernel's do without
contraction, in the kernel's order), the Huber weights in f64 arithmetic, the 15 sums folded in the stated partition with a
thread's terms added in ascending trip and, within a trip, in ascending submap, and `localize`'s choice.  It builds on
tests/scan_registration_ref.py (the neighbour gather, trilinear and its gradient, the block fold, the trust-region loop) and
on tests/map_query_ref.py's pose rule and layer view.  `evaluate_map(..., FT=np.float64)` runs the same formulas in f64 (the
Jacobian check's reference).  Test infrastructure: not part of the product."""
import math
import types

import numpy as np

from tests import scan_registration_ref as SR
from tests.map_query_ref import QueryLayer
from tests.projected_map_ref import F, inverse, quat_rotate

QUOTA, THREADS, TRIPS, FOLD = SR.QUOTA, SR.THREADS, SR.TRIPS, SR.FOLD
PAIRS = SR.PAIRS


def map_config(layer="esdf", huber_delta_m=math.inf, score_point_stride=1):
    return types.SimpleNamespace(layer=layer, huber_delta_m=F(huber_delta_m), score_point_stride=int(score_point_stride))


class Map:
    """posed finished submaps: `submaps` anything with voxel_size, vps, block_index and the raw arrays of the chosen layer
    (oracle.synth.SubmapData); `poses` T_M_S [n][7] f32.  T_S_M once in f32 by map_query_ref's rule."""

    def __init__(self, submaps, poses, layer="esdf"):
        self.layers = [QueryLayer(sm, layer) for sm in submaps]
        self.T_M_S = np.asarray(poses, F).reshape(-1, 7)
        assert len(self.T_M_S) == len(self.layers)
        self.T_S_M = [inverse(T) for T in self.T_M_S]


def _mission_points(pc, T, delta, FT):
    """q = R_prior p_C and p_M, both [m][3] in FT, with c and s"""
    T = np.asarray(T, F).reshape(7)
    delta = [float(v) for v in delta]
    c, s = FT(math.cos(delta[3])), FT(math.sin(delta[3]))
    t = [FT(float(T[4 + a]) + delta[a]) for a in range(3)]
    q = quat_rotate(T[:4], pc) if FT is F else SR.quat_rotate_any(T[:4].astype(FT), pc.astype(FT))
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    return q, np.stack([(c * qx - s * qy) + t[0], (s * qx + c * qy) + t[1], qz + t[2]], -1).astype(FT), c, s


def _submap_terms(M, k, pm, q, c, s, max_abs_distance, FT, want_J):
    """submap k at mission-frame points pm [m][3] -> (usable [m], r [m], J [m][4] or None); rows not usable hold zeros"""
    L = M.layers[k]
    qi, ti = M.T_S_M[k]
    if FT is F:
        p = (quat_rotate(qi, pm) + ti).astype(F)
    else:
        p = (SR.quat_rotate_any(qi.astype(FT), pm) + ti.astype(FT)).astype(FT)
    inside = (np.abs((p * FT(L.bs_inv)).astype(FT)) < FT(SR.LIMIT)).all(1)
    p = np.where(inside[:, None], p, FT(0)).astype(FT)  # (kept out of the integer casts; masked below)
    ok, d8, dl = SR._neighbours(L, p, FT)
    r = SR.trilinear(d8, dl).astype(FT)
    usable = inside & ok & (np.abs(r) < FT(max_abs_distance))
    J = None
    if want_J:
        gl = SR.trilinear_gradient(d8, dl)
        gs = np.stack([(ga * FT(L.vs_inv)).astype(FT) for ga in gl], -1)
        qm = M.T_M_S[k][:4]
        g = quat_rotate(qm, gs) if FT is F else SR.quat_rotate_any(qm.astype(FT), gs)
        qx, qy = q[:, 0], q[:, 1]
        j3 = (g[:, 0] * ((-s) * qx - c * qy) + g[:, 1] * (c * qx - s * qy)).astype(FT)
        J = np.where(usable[:, None], np.stack([g[:, 0], g[:, 1], g[:, 2], j3], -1), FT(0)).astype(FT)
    return usable, np.where(usable, r, FT(0)).astype(FT), J


def huber(r, a):
    """(rho [m], w [m]) in f64 from residuals r (any float dtype) and the scale a: arithmetic alone"""
    rd, a = np.asarray(r).astype(np.float64), np.float64(a)
    ar = np.abs(rd)
    with np.errstate(all="ignore"):
        inl = ar <= a
        w = np.where(inl, 1.0, a / ar)
        rho = np.where(inl, rd * rd, (2.0 * a) * ar - a * a)
    return rho, w


def fold(terms, swap_submaps=False):
    """terms [K][m][k] (per submap one row per strided candidate slot j, zeros where nothing is added) -> [k]: a thread adds
    in ascending trip and within a trip in ascending submap; then scan_registration_ref's block fold and partial fold.
    swap_submaps: the WRONG order of the mutation check (submaps 1, 0, ...)."""
    K, m, k = terms.shape
    if m == 0:
        return np.zeros(k, terms.dtype)
    groups = -(-m // QUOTA)
    pad = np.zeros((K, groups * QUOTA, k), terms.dtype)
    pad[:, :m] = terms
    t = pad.reshape(K, groups, TRIPS, THREADS, k)
    order = list(range(K))
    if swap_submaps and K > 1:
        order[0], order[1] = 1, 0
    acc = np.zeros((groups, THREADS, k), terms.dtype)
    for trip in range(TRIPS):
        for sub in order:
            acc = acc + t[sub, :, trip]
    partials = SR._block_fold(acc)
    rounds = -(-groups // FOLD)
    padp = np.zeros((rounds * FOLD, k), terms.dtype)
    padp[:groups] = partials
    pp = padp.reshape(rounds, FOLD, k)
    acc = np.zeros((FOLD, k), terms.dtype)
    for rnd in range(rounds):
        acc = acc + pp[rnd]
    return SR._block_fold(acc[None])[0]


def _candidates(points, cfg, stride):
    """the strided points [m][3] and which of them pass the range gate"""
    pc = np.asarray(points, F).reshape(-1, 3)[::stride]
    with np.errstate(all="ignore"):
        range2 = ((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2]).astype(F)
        cand = (range2 >= F(cfg.min_range_m * cfg.min_range_m)) & (range2 <= F(cfg.max_range_m * cfg.max_range_m))
    return pc, cand


def point_terms_map(M, points, T, delta, cfg, FT=F, want_J=True):
    """-> (cand [m], [(usable, r, J) per submap]) over the strided points; cfg.point_stride is the stride"""
    pc, cand = _candidates(points, cfg, cfg.point_stride)
    with np.errstate(all="ignore"):
        q, pm, c, s = _mission_points(pc, T, delta, FT)
        per = []
        for k in range(len(M.layers)):
            u, r, J = _submap_terms(M, k, pm, q, c, s, cfg.max_abs_distance_m, FT, want_J)
            u = u & cand
            r = np.where(u, r, FT(0)).astype(FT)
            if J is not None:
                J = np.where(u[:, None], J, FT(0)).astype(FT)
            per.append((u, r, J))
    return cand, per


def _terms15(r, J, usable, a):
    rd, Jd = r.astype(np.float64), J.astype(np.float64)
    rho, w = huber(rd, a)
    t = np.zeros((len(rd), 15))
    t[:, 0] = np.where(usable, rho, 0.0)
    wr = w * rd
    for k in range(4):
        t[:, 1 + k] = Jd[:, k] * wr
    for e, (k, l) in enumerate(PAIRS):
        t[:, 5 + e] = (w * Jd[:, k]) * Jd[:, l]
    return t


def map_terms(M, points, T, delta, cfg, mcfg, FT=F):
    """-> (terms [K][m][15] f64, usable [K][m], cand [m]) over the strided points: what `totals` folds.  A point's terms do
    not depend on the other points, so a prefix of the scan is a prefix of these rows."""
    cand, per = point_terms_map(M, points, T, delta, cfg, FT)
    terms = np.stack([_terms15(r, J, u, mcfg.huber_delta_m) for u, r, J in per])
    return terms, np.stack([u for u, _, _ in per]), cand


def totals(terms, usable, cand, m=None, swap_submaps=False):
    """the first m strided slots (all by default) -> (out [15] f64, n_terms, n_points_valid, n_candidates)"""
    m = terms.shape[1] if m is None else m
    u = usable[:, :m]
    return fold(terms[:, :m], swap_submaps), int(u.sum()), int(u.any(0).sum()), int(cand[:m].sum())


def evaluate_map(M, points, T, delta, cfg, mcfg, FT=F, swap_submaps=False):
    """vgx_scan_registration_evaluate_map -> (out [15] f64, n_terms, n_points_valid, n_candidates)"""
    return totals(*map_terms(M, points, T, delta, cfg, mcfg, FT), swap_submaps=swap_submaps)


def score_poses(M, points, poses, cfg, mcfg, chunk=128):
    """vgx_scan_registration_score_poses -> (cost [P] f64, n_terms [P], n_points_valid [P], n_candidates [P]): per pose the
    cost-only evaluation at delta = 0 with score_point_stride.  The submap part runs over `chunk` poses at a time (a point's
    arithmetic does not depend on its neighbours in the array); the fold is per pose."""
    poses = np.asarray(poses, F).reshape(-1, 7)
    P, K = len(poses), len(M.layers)
    pc, cand = _candidates(points, cfg, mcfg.score_point_stride)
    m = len(pc)
    cost, nt, nv = np.zeros(P), np.zeros(P, np.int64), np.zeros(P, np.int64)
    nc = np.full(P, int(cand.sum()), np.int64)
    zero = [0.0] * 4
    with np.errstate(all="ignore"):
        for p0 in range(0, P, chunk):
            Ts = poses[p0:p0 + chunk]
            pm = np.concatenate([_mission_points(pc, T, zero, F)[1] for T in Ts]) if m else np.zeros((0, 3), F)
            candc = np.tile(cand, len(Ts))
            rho = np.zeros((K, len(Ts), m, 1))
            usable = np.zeros((K, len(Ts), m), bool)
            for k in range(K):
                u, r, _ = _submap_terms(M, k, pm, None, None, None, cfg.max_abs_distance_m, F, False)
                u = u & candc
                rho[k, :, :, 0] = np.where(u, huber(r, mcfg.huber_delta_m)[0], 0.0).reshape(len(Ts), m)
                usable[k] = u.reshape(len(Ts), m)
            for i in range(len(Ts)):
                cost[p0 + i] = 0.5 * fold(rho[:, i])[0]
                nt[p0 + i] = int(usable[:, i].sum())
                nv[p0 + i] = int(usable[:, i].any(0).sum())
    return cost, nt, nv, nc


def _loop_evaluate(Mm, points, T, x, cfg):
    """scan_registration_ref.evaluate's signature over a (map, map config) pair: the loop sees n_points_valid"""
    out, _, nv, nc = evaluate_map(Mm[0], points, T, x, cfg, Mm[1])
    return out, nv, nc


# scan_registration_ref.refine's own loop, its evaluation bound to the map's (the function's code, other globals)
_refine_loop = types.FunctionType(SR.refine.__code__, dict(vars(SR), evaluate=_loop_evaluate), "refine_map", SR.refine.__defaults__)


def refine_map(M, points, T, cfg, mcfg, **kw):
    """vgx_scan_registration_refine_map -> (T_refined [7] f32, delta [4], summary dict, history list of dicts)"""
    return _refine_loop((M, mcfg), points, T, cfg, **kw)


def choose(cost, n_terms, n_points_valid, n_candidates, min_valid_ratio):
    """localize's choice: the lowest cost / n_terms among the eligible poses, ties to the lowest index; -1 if none"""
    best, best_score = -1, 0.0
    for m in range(len(cost)):
        if not (n_candidates[m] > 0 and float(n_points_valid[m]) / float(n_candidates[m]) >= float(min_valid_ratio)):
            continue
        with np.errstate(all="ignore"):
            score = float(np.float64(cost[m]) / np.float64(n_terms[m]))
        if best < 0 or score < best_score:
            best, best_score = m, score
    return best


def localize(M, points, poses, cfg, mcfg, scores=None, **kw):
    """vgx_scan_registration_localize -> (best_index, T_refined, delta, summary, history); `scores`: score_poses' result
    where the caller already has it"""
    poses = np.asarray(poses, F).reshape(-1, 7)
    scores = scores if scores is not None else score_poses(M, points, poses, cfg, mcfg)
    best = choose(*scores, cfg.min_valid_ratio)
    if best < 0:
        summary = dict(usable=0, termination=SR.TOO_FEW_POINTS, num_iterations=0, num_successful_steps=0, num_evaluations=0,
                       num_factorization_failures=0, n_candidates=0, n_valid_first=0, n_valid_last=0, initial_cost=0.0, final_cost=0.0)
        return -1, poses[0].copy(), np.zeros(4), summary, []
    return (best,) + refine_map(M, points, poses[best], cfg, mcfg, **kw)


def hypothesis_grid(xs, ys, n_yaw, z):
    """poses [len(xs) len(ys) n_yaw][7] f32, x-major then y then yaw = 2 pi k / n_yaw: SR.pose7 of each"""
    return np.array([SR.pose7((x, y, z, 2.0 * math.pi * k / n_yaw)) for x in xs for y in ys for k in range(n_yaw)], F)
