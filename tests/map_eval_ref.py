"""CPU restatement of vgx_tsdf_layer_transform_submap and vgx_evaluate_layers_rmse (include/voxgraph_amd.h):
voxblox's transformLayer into an empty layer and evaluateLayersRmse, vectorised in numpy.  f32 ops round once each, in
the kernels' order; the f64 sum of squared errors follows the association the header states, so both results are
comparable with the device's bit for bit.

A layer here is (block_index [n][3], distance [n][vps^3], observed bool [n][vps^3]) in slot order."""
import numpy as np

from tests import projected_map_ref as P

F = np.float32
MODES = ALL_VOXELS, IGNORE_BEHIND_TEST, IGNORE_BEHIND_GT, IGNORE_BEHIND_ALL = 0, 1, 2, 3
TSDF_OBSERVED_WEIGHT = F(1e-6)


def transform_layer(sm, T_L_S):
    """transformLayer(sm's TSDF layer, T_L_S, empty layer): {(bx, by, bz): (distance, weight)}.  A block is kept iff one
    of its voxel centres interpolates; an interpolated voxel is copied as {d, w}, every other voxel of it is (0, 0)."""
    vps, vs = int(sm.vps), F(sm.voxel_size)
    raw = P.RawLayer(sm)
    qi, ti = P.inverse(T_L_S)
    cand = P.candidate_blocks(raw, T_L_S, vps, vs)
    out = {}
    for s in range(0, len(cand), 256):
        part = cand[s:s + 256]
        ok, d, w = raw.interp(P.transform(qi, ti, P.block_centres(part, vps, vs)))
        for b, o, db, wb in zip(part, ok, d, w):
            if o.any():
                out[tuple(int(v) for v in b)] = (np.where(o, db, F(0)).astype(F), np.where(o, wb, F(0)).astype(F))
    return out


def esdf_layer(block_index, distance, observed):
    """[n][vps^3] arrays (2-D, also when n = 0)"""
    return np.asarray(block_index, np.int64).reshape(-1, 3), np.asarray(distance, F), np.asarray(observed) != 0


def tsdf_layer(block_index, distance, weight):
    return np.asarray(block_index, np.int64).reshape(-1, 3), np.asarray(distance, F), np.asarray(weight, F) > TSDF_OBSERVED_WEIGHT


def _threads(vps):
    return 256 if vps == 16 else 128


def _wave_tree_then_waves(v):
    """[..., T] per-thread values -> the __shfl_down tree inside each wave of 64, then the waves in order."""
    w = v.reshape(v.shape[:-1] + (-1, 64)).copy()
    o = 32
    while o:
        w[..., :o] = w[..., :o] + w[..., o:2 * o]
        o //= 2
    lane0 = w[..., 0]
    acc = lane0[..., 0].copy()
    for i in range(1, lane0.shape[-1]):
        acc = acc + lane0[..., i]
    return acc


def block_sums(sq, vps):
    """[m, vps^3] f64 squared errors (0 where not evaluated) -> [m] per-block sums in the kernel's association:
    voxel v = 4 (t + T k) + j summed by thread t, k outer, j inner, from 0.0."""
    T = _threads(vps)
    K = vps ** 3 // (4 * T)
    x = sq.reshape(len(sq), K, T, 4)
    s = np.zeros((len(sq), T), np.float64)
    for k in range(K):
        for j in range(4):
            s = s + x[:, k, :, j]
    return _wave_tree_then_waves(s)


def fold_sums(partials):
    """per-test-block sums in slot order -> the total: block b to thread b mod 1024 in ascending b from 0.0, then the
    wave tree and the 16 waves in order."""
    p = np.asarray(partials, np.float64)
    r = -(-len(p) // 1024) if len(p) else 0
    pad = np.zeros(r * 1024, np.float64)
    pad[:len(p)] = p
    s = np.zeros(1024, np.float64)
    for i in range(r):
        s = s + pad[i * 1024:(i + 1) * 1024]
    return float(_wave_tree_then_waves(s))


def evaluate_layers_rmse(gt, test, mode, vps):
    """evaluateLayersRmse(gt, test, mode) -> (details dict, error layer (block_index, distance, set))."""
    gbi, gd, go = gt
    tbi, td, to = test
    nv = vps ** 3
    gslot = {tuple(int(c) for c in b): i for i, b in enumerate(gbi)}
    tkeys = {tuple(int(c) for c in b) for b in tbi}
    match = np.array([gslot.get(tuple(int(c) for c in b), -1) for b in tbi], np.int64)
    has = match >= 0
    non = nv * int((~has).sum()) + nv * sum(1 for b in gbi if tuple(int(c) for c in b) not in tkeys)
    g = match[has]
    dg, og = gd[g], go[g]
    dt, ot = td[has], to[has]
    observed = og & ot
    ign_test = mode in (IGNORE_BEHIND_TEST, IGNORE_BEHIND_ALL)
    ign_gt = mode in (IGNORE_BEHIND_GT, IGNORE_BEHIND_ALL)
    ignored = observed & ((ign_test & (dt < F(0))) | (ign_gt & (dg < F(0))))
    evaluated = observed & ~ignored
    e = np.where(evaluated, (dt - dg).astype(F), F(0)).astype(F)
    sq = np.where(evaluated, (e * e).astype(F).astype(np.float64), 0.0)
    partial = np.zeros(len(tbi), np.float64)
    partial[has] = block_sums(sq, vps) if has.any() else []
    total = fold_sums(partial)
    n_eval, n_ign = int(evaluated.sum()), int(ignored.sum())
    non += int((~observed).sum())
    ae = np.abs(e[evaluated])
    details = {
        "rmse": float(F(np.sqrt(total / n_eval))) if n_eval else 0.0,
        "max_error": float(ae.max()) if n_eval else 0.0,
        "min_error": 0.0,
        "total_squared_error": total,
        "min_abs_error": float(ae.min()) if n_eval else 0.0,
        "num_evaluated_voxels": n_eval,
        "num_ignored_voxels": n_ign,
        "num_overlapping_voxels": n_eval + n_ign,
        "num_non_overlapping_voxels": non,
    }
    return details, (tbi[has].astype(np.int32), e, evaluated.astype(np.uint8))
