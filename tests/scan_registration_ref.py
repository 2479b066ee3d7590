"""Sequential restatement of scan-to-map registration (include/voxgraph_amd.h, "Scan-to-map registration"):
the formulation in numpy f32 -- every numpy op rounds once, as the kernel's do without contraction, in the kernel's order --
the 15 f64 sums folded in the stated partition (1024 candidates per workgroup, 256 threads of 4 trips, the wave tree, the
waves in order, the 256-wide fold), and the trust-region loop with tests/pose_graph_ref.py's Cholesky and substitutions.
math.sin / math.cos are the libm the library's host code calls.  `evaluate(..., FT=np.float64)` runs the same formulas in
f64 (the Jacobian check's reference).  Test infrastructure: not part of the product."""
import math
import time
import types

import numpy as np

from tests import pose_graph_ref as pg
from tests.projected_map_ref import EPS, F, RawLayer, quat_rotate

LIMIT = 2.0 ** 30
QUOTA, THREADS, TRIPS, FOLD = 1024, 256, 4, 256
TOO_FEW_POINTS = "too_few_points"


def config(max_abs_distance_m, min_range_m=0.0, max_range_m=math.inf, point_stride=1, min_valid_ratio=0.5):
    return types.SimpleNamespace(min_range_m=F(min_range_m), max_range_m=F(max_range_m), max_abs_distance_m=F(max_abs_distance_m),
                                 point_stride=int(point_stride), min_valid_ratio=F(min_valid_ratio))


def layer_of(voxel_size, vps, block_index, distance, weight):
    """a RawLayer (block lookup, f32 constants) from a layer's download"""
    nv = int(vps) ** 3
    return RawLayer(types.SimpleNamespace(vps=vps, voxel_size=voxel_size, block_index=np.asarray(block_index).reshape(-1, 3),
                                          tsdf_distance=np.asarray(distance, F).reshape(-1, nv),
                                          tsdf_weight=np.asarray(weight, F).reshape(-1, nv)))


def _neighbours(L, p, FT):
    """interp_base + the 8 gathers at points [m][3] (FT) -> (ok, d8 list of 8 [m], (dl0, dl1, dl2))"""
    vps = L.vps
    vs, vs_inv, bs, bs_inv, eps = FT(L.vs), FT(L.vs_inv), FT(L.bs), FT(L.bs_inv), FT(EPS)
    blk, vox, dl = [], [], []
    for a in range(3):
        pa = p[:, a]
        b0 = np.floor((pa * bs_inv) + eps).astype(np.int64)
        origin = (b0.astype(FT) * bs).astype(FT)
        v = np.clip(np.floor(((pa - origin) * vs_inv) + eps).astype(np.int64), 0, vps - 1)
        centre = (origin + ((v.astype(FT) + FT(0.5)) * vs)).astype(FT)
        v = np.where((pa - centre) < FT(0), v - 1, v)
        wrap = v < 0
        b0 = np.where(wrap, b0 - 1, b0)
        v = np.where(wrap, v + vps, v)
        origin2 = (b0.astype(FT) * bs).astype(FT)
        dl.append(((pa - (origin2 + ((v.astype(FT) + FT(0.5)) * vs))) * vs_inv).astype(FT))
        blk.append(b0)
        vox.append(v)
    ok = np.ones(len(p), bool)
    d8 = []
    for k in range(8):
        off = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        nb, nv = [], []
        for a in range(3):
            v = vox[a] + off[a]
            nb.append(np.where(v >= vps, blk[a] + 1, blk[a]))
            nv.append(np.where(v >= vps, v - vps, v))
        s = L.slot(np.stack(nb, -1))
        lin = nv[0] + vps * (nv[1] + vps * nv[2])
        sc = np.maximum(s, 0)
        dk = np.where(s >= 0, L.d[sc, lin] if L.d.size else F(0), F(0)).astype(FT)
        wk = np.where(s >= 0, L.w[sc, lin] if L.w.size else F(0), F(0)).astype(F)
        ok &= (s >= 0) & (wk > F(0))
        d8.append(dk)
    return ok, d8, dl


def _coefficients(v):
    c1 = -v[0] + v[4]
    c2 = -v[0] + v[2]
    c3 = -v[0] + v[1]
    c4 = ((v[0] - v[2]) - v[4]) + v[6]
    c5 = ((v[0] - v[1]) - v[2]) + v[3]
    c6 = ((v[0] - v[1]) - v[4]) + v[5]
    c7 = ((((((-v[0] + v[1]) + v[2]) - v[3]) + v[4]) - v[5]) - v[6]) + v[7]
    return v[0], c1, c2, c3, c4, c5, c6, c7


def trilinear(v, dl):
    """interp_trilinear"""
    x, y, z = dl
    c0, c1, c2, c3, c4, c5, c6, c7 = _coefficients(v)
    q4, q5, q6, q7 = x * y, y * z, z * x, (x * y) * z
    return ((((((c0 + x * c1) + y * c2) + z * c3) + q4 * c4) + q5 * c5) + q6 * c6) + q7 * c7


def trilinear_gradient(v, dl):
    """interp_trilinear_gradient: d / d dl, every sum left to right"""
    x, y, z = dl
    _, c1, c2, c3, c4, c5, c6, c7 = _coefficients(v)
    return (((c1 + y * c4) + z * c6) + (y * z) * c7,
            ((c2 + x * c4) + z * c5) + (z * x) * c7,
            ((c3 + y * c5) + x * c6) + (x * y) * c7)


def point_terms(L, points, T, delta, cfg, FT=F):
    """Per point of the scan [n][3]: (candidate [n] bool, usable [n] bool, r [n], J [n][4]) in FT; rows that are not
    usable hold zeros.  T the f32 prior {qw,qx,qy,qz,tx,ty,tz}, delta 4 Python floats."""
    pc = np.asarray(points, F).reshape(-1, 3)
    n = len(pc)
    T = np.asarray(T, F).reshape(7)
    delta = [float(v) for v in delta]
    with np.errstate(all="ignore"):
        idx = np.arange(n)
        range2 = ((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2]).astype(F)
        min2, max2 = F(cfg.min_range_m * cfg.min_range_m), F(cfg.max_range_m * cfg.max_range_m)
        cand = (idx % cfg.point_stride == 0) & (range2 >= min2) & (range2 <= max2)
        if FT is F:
            c, s = F(math.cos(delta[3])), F(math.sin(delta[3]))
            t = [F(float(T[4 + a]) + delta[a]) for a in range(3)]
            q = quat_rotate(T[:4], pc)
        else:
            c, s = FT(math.cos(delta[3])), FT(math.sin(delta[3]))
            t = [FT(float(T[4 + a]) + delta[a]) for a in range(3)]
            q = quat_rotate_any(T[:4].astype(FT), pc.astype(FT))
        qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
        p = np.stack([(c * qx - s * qy) + t[0], (s * qx + c * qy) + t[1], qz + t[2]], -1).astype(FT)
        inside = (np.abs((p * FT(L.bs_inv)).astype(FT)) < FT(LIMIT)).all(1)
        p = np.where(inside[:, None], p, FT(0)).astype(FT)  # (kept out of the integer casts; masked below)
        ok, d8, dl = _neighbours(L, p, FT)
        r = trilinear(d8, dl).astype(FT)
        usable = cand & inside & ok & (np.abs(r) < FT(cfg.max_abs_distance_m))
        gl = trilinear_gradient(d8, dl)
        g = [(ga * FT(L.vs_inv)).astype(FT) for ga in gl]
        j3 = (g[0] * ((-s) * qx - c * qy) + g[1] * (c * qx - s * qy)).astype(FT)
        J = np.stack([g[0], g[1], g[2], j3], -1).astype(FT)
    r = np.where(usable, r, FT(0)).astype(FT)
    J = np.where(usable[:, None], J, FT(0)).astype(FT)
    return cand, usable, r, J


def quat_rotate_any(q, v):
    """projected_map_ref.quat_rotate in the dtype of its arguments"""
    w, x, y, z = q
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    u0 = y * v2 - z * v1
    u1 = z * v0 - x * v2
    u2 = x * v1 - y * v0
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    c0 = y * u2 - z * u1
    c1 = z * u0 - x * u2
    c2 = x * u1 - y * u0
    return np.stack([(v0 + w * u0) + c0, (v1 + w * u1) + c1, (v2 + w * u2) + c2], -1)


def _wave_tree(v):
    """[..., 64, k] -> [..., k]: v[l] += v[l + o], o = 32 .. 1"""
    v = v.copy()
    o = 32
    while o > 0:
        v[..., :o, :] = v[..., :o, :] + v[..., o:2 * o, :]
        o >>= 1
    return v[..., 0, :]


def _block_fold(v):
    """[groups][256][k] per-thread sums -> [groups][k]: the wave tree, then the 4 waves in order"""
    w = _wave_tree(v.reshape(v.shape[0], 4, 64, v.shape[-1]))
    out = w[:, 0]
    for i in range(1, 4):
        out = out + w[:, i]
    return out


def fold(terms, swap_partials=None):
    """terms [m][k] (one row per strided candidate slot j, zeros where nothing is added) -> [k], in the contract's order.
    swap_partials=(a, b): the WRONG order of the mutation check."""
    m, k = terms.shape
    if m == 0:
        return np.zeros(k, terms.dtype)
    groups = -(-m // QUOTA)
    pad = np.zeros((groups * QUOTA, k), terms.dtype)
    pad[:m] = terms
    t = pad.reshape(groups, TRIPS, THREADS, k)
    acc = np.zeros((groups, THREADS, k), terms.dtype)
    for trip in range(TRIPS):
        acc = acc + t[:, trip]
    partials = _block_fold(acc)
    if swap_partials:
        a, b = swap_partials
        partials[[a, b]] = partials[[b, a]]
    rounds = -(-groups // FOLD)
    padp = np.zeros((rounds * FOLD, k), terms.dtype)
    padp[:groups] = partials
    pp = padp.reshape(rounds, FOLD, k)
    acc = np.zeros((FOLD, k), terms.dtype)
    for rnd in range(rounds):
        acc = acc + pp[rnd]
    return _block_fold(acc[None])[0]


PAIRS = [(k, l) for k in range(4) for l in range(k, 4)]


def evaluate(L, points, T, delta, cfg, FT=F):
    """vgx_scan_registration_evaluate -> (out [15] f64, n_valid, n_candidates)"""
    cand, usable, r, J = point_terms(L, points, T, delta, cfg, FT)
    sel = slice(None, None, cfg.point_stride)
    rd, Jd = r[sel].astype(np.float64), J[sel].astype(np.float64)
    terms = np.empty((len(rd), 15))
    terms[:, 0] = rd * rd
    for k in range(4):
        terms[:, 1 + k] = Jd[:, k] * rd
    for e, (k, l) in enumerate(PAIRS):
        terms[:, 5 + e] = Jd[:, k] * Jd[:, l]
    return fold(terms), int(usable.sum()), int(cand.sum())


def system(out):
    g = np.array(out[1:5], np.float64)
    H = np.zeros((4, 4))
    for e, (k, l) in enumerate(PAIRS):
        H[k, l] = H[l, k] = out[5 + e]
    return g, H


def refined_pose(T, delta):
    """q_z(yaw) (x) q_prior, t_prior + delta in f64 from the f32 prior, rounded once"""
    T = np.asarray(T, F).reshape(7)
    cz, sz = math.cos(0.5 * delta[3]), math.sin(0.5 * delta[3])
    w, x, y, z = (float(v) for v in T[:4])
    out = [cz * w - sz * z, cz * x - sz * y, cz * y + sz * x, cz * z + sz * w]
    out += [float(T[4 + a]) + float(delta[a]) for a in range(3)]
    return np.array(out, np.float64).astype(F)


def refine(L, points, T, cfg, parameter_tolerance=3e-3, function_tolerance=1e-6, gradient_tolerance=1e-10, max_num_iterations=50,
           max_solver_time_in_seconds=4.0, initial_trust_region_radius=1e4):
    """vgx_scan_registration_refine -> (T_refined [7] f32, delta [4], summary dict, history list of dicts)"""
    t0 = time.perf_counter()
    T = np.asarray(T, F).reshape(7)
    evaluations = [0]

    def full(x):
        evaluations[0] += 1
        out, nv, nc = evaluate(L, points, T, x, cfg)
        g, H = system(out)
        return 0.5 * out[0], g, H, nv, nc

    def enough(nv, nc):
        return nc > 0 and nv / nc >= float(cfg.min_valid_ratio)

    x = [0.0, 0.0, 0.0, 0.0]
    cost, g, H, nv, nc = full(x)
    summary = dict(n_candidates=nc, n_valid_first=nv, initial_cost=cost)
    history = []
    it, successful, failures = 0, 0, 0
    enough_first = enough(nv, nc)
    reason = "max_iterations"
    if not enough_first:
        reason = TOO_FEW_POINTS
    else:
        radius, decrease = float(initial_trust_region_radius), 2.0
        while it < max_num_iterations:
            it += 1
            rec = dict(cost=cost, trial_cost=0.0, gain_ratio=0.0, radius=radius, step_norm=0.0, accepted=0, factorization_failed=0)
            history.append(rec)
            if np.abs(g).max() <= gradient_tolerance:
                reason = "gradient_tolerance"
                break
            d2 = np.clip(np.diag(H), 1e-6, 1e32)
            A = H.copy()
            A[np.arange(4), np.arange(4)] = np.diag(H) + d2 / radius
            try:
                z, _ = pg.spd_solve(A, g)
            except pg.NotPositiveDefinite:
                rec["factorization_failed"] = 1
                failures += 1
                radius /= decrease
                decrease *= 2.0
                continue
            step = -z
            Hs = pg.matvec(H, step)
            step_norm = math.sqrt(pg.dot(step, step))
            rec["step_norm"] = step_norm
            if step_norm <= parameter_tolerance * (math.sqrt(pg.dot(x, x)) + parameter_tolerance):
                reason = "parameter_tolerance"
                break
            cand = [float(x[i]) + float(step[i]) for i in range(4)]
            cand[3] = pg.normalize_angle(cand[3])
            trial, gt, Ht, nvt, _ = full(cand)
            model_decrease = -(pg.dot(g, step) + 0.5 * pg.dot(step, Hs))
            rho = (cost - trial) / model_decrease if model_decrease > 0.0 else -1.0
            rec["trial_cost"], rec["gain_ratio"] = trial, rho
            if rho > 1e-3:
                rec["accepted"] = 1
                successful += 1
                rel = abs(cost - trial) / max(cost, 1e-300)
                x, cost, g, H, nv = cand, trial, gt, Ht, nvt
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
    converged = reason in ("parameter_tolerance", "function_tolerance", "gradient_tolerance")
    usable = bool(converged and enough_first and enough(nv, nc))
    summary.update(usable=int(usable), termination=reason, num_iterations=it, num_successful_steps=successful,
                   num_evaluations=evaluations[0], num_factorization_failures=failures, n_valid_last=nv, final_cost=cost)
    return (refined_pose(T, x) if usable else T.copy()), np.array(x, np.float64), summary, history


# ---------------------------------------------------------------------------
# the scene the CPU and GPU tests share: __graft_entry__.smoke()'s box room seen by a 256 x 16 beam scanner
# ---------------------------------------------------------------------------
ROOM_LO, ROOM_HI = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])
VOXEL_SIZE, VPS, MAX_ABS_DISTANCE = 0.2, 16, 0.55
PRIOR_OFF = np.array([0.15, 0.15, 0.10, math.radians(3.0)])     # a prior is off by up to this: x y z yaw


def scan_pose(k):
    """(x, y, z, yaw) of scan k: six scans build the layer, the seventh (k = 6) is registered"""
    return np.array([0.1 + 0.15 * k, -0.05 + 0.05 * k, 0.02, 0.03 * k])


def pose7(p4):
    """(x, y, z, yaw) -> T_S_C {qw,qx,qy,qz, tx,ty,tz} f32"""
    return np.array([math.cos(0.5 * p4[3]), 0.0, 0.0, math.sin(0.5 * p4[3]), p4[0], p4[1], p4[2]], F)


def room_scan(p4, n_az=256, n_el=16):
    """the sensor-frame points [n_az n_el][3] f32 a scanner at pose p4 sees of the box room (no axis-aligned beam)"""
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, n_az, endpoint=False) + (2 * np.pi / n_az) / 3.0,
                         np.linspace(-0.3, 0.3, n_el) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    c, s = math.cos(p4[3]), math.sin(p4[3])
    dw = np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1], d[:, 2]], -1)
    lo, hi = ROOM_LO - p4[:3], ROOM_HI - p4[:3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dw > 0, hi / dw, np.where(dw < 0, lo / dw, np.inf)).min(1)
    return (d * t[:, None]).astype(F)


def seeded_prior(seed):
    """the seventh scan's true pose off by up to PRIOR_OFF -> (x, y, z, yaw)"""
    rng = np.random.default_rng(1000 + seed)
    return scan_pose(6) + rng.uniform(-1, 1, 4) * PRIOR_OFF


def pose_error(T, p4_true):
    """(translation error in m, yaw error in rad) of a 7-vector pose against a true (x, y, z, yaw)"""
    T = np.asarray(T, np.float64)
    yaw = 2.0 * math.atan2(T[3], T[0])
    return float(np.linalg.norm(T[4:7] - p4_true[:3])), abs(pg.normalize_angle(yaw - float(p4_true[3])))


_ROOM = []


def room_layer_arrays():
    """(block_index, distance, weight) of the layer the CPU oracle's FastTsdfIntegrator builds from scans 0..5 with
    voxgraph's configuration; computed once and shared (nobody writes to it)"""
    if not _ROOM:
        from oracle import pyoracle as orc
        layer = orc.TsdfLayer(VOXEL_SIZE, VPS)
        integrator = orc.FastTsdfIntegrator(orc.voxgraph_tsdf_config(), layer)
        for k in range(6):
            integrator.integratePointCloud(pose7(scan_pose(k)), room_scan(scan_pose(k)))
        bi, d, w, _ = layer.download()
        for a in (bi, d, w):
            a.setflags(write=False)
        _ROOM.append((bi, d, w))
    return _ROOM[0]


def room_layer():
    bi, d, w = room_layer_arrays()
    return layer_of(VOXEL_SIZE, VPS, bi, d, w)


def plane_layer(z0=0.3):
    """a single horizontal plane: D = z - z0 at every voxel of a 2 x 2 x 2 block box around the origin, weight 1"""
    from oracle import synth
    bi = synth.dense_block_index((-1, -1, -1), (2, 2, 2)).astype(np.int32)
    nv = VPS ** 3
    i = np.arange(nv)
    zc = (bi[:, 2:3].astype(F) * F(F(VPS) * F(VOXEL_SIZE)) + ((i // (VPS * VPS)).astype(F)[None] + F(0.5)) * F(VOXEL_SIZE)).astype(F)
    d = (zc - F(z0)).astype(F)
    return bi, d, np.ones_like(d)
