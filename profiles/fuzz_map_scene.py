"""The scene generator of the map-product fuzzers (profiles/fuzz_map_layers.py, profiles/fuzz_map_meshes.py) and of
tests/test_fuzz_map_cpu.py.  numpy and oracle/synth.py only: importable without a GPU and without the library.

draw(seed) gives one Scene from one np.random.default_rng(seed).  The categorical classes (voxel size, pose kind of
the first submap, min_weight, weld-threshold kinds, evaluation layer x mode, query flags x pose) follow the seed round
robin, so that a short run of consecutive seeds draws each of them; everything else comes from the generator.
Scene.drawn reports the classes a seed drew: tests/test_fuzz_map_cpu.py tallies it over the suite's seed ranges.

Geometry: every submap's blocks lie in a small box around one common block offset `offset` (a few tens of blocks from
the origin, either sign), in the submap frame.  A pose is a rotation about the scene centre c = (offset + 1) * block_size
plus a small shift, T x = R (x - c) + c + shift, so that the posed submaps overlap in the layer wherever the offset is
and the translation R-dependent part (c - R c) is large: f32 coordinates of tens of metres, index arithmetic of both
signs."""
import types

import numpy as np

from oracle import synth

F = np.float32
VOXEL_SIZES = (0.05, 0.1, 0.2, 0.125, 0.25, 0.137)          # round decimals, dyadic (exact f32 products), one odd value
POSE_KINDS = ("identity", "yaw", "full", "near_identity", "quarter_turn", "grid_shift")
MIN_WEIGHTS = (0.0, 1e-4, 0.5, 1.0)
THRESHOLD_KINDS = ("default", "half_voxel", "voxel", "block", "extent", "log_uniform")
VALUE_KINDS = ("sphere", "ground", "truncated", "noise")
SHAPE_KINDS = ("box", "one_block", "slab")
EVAL_COMBOS = tuple((layer, mode) for layer in (0, 1) for mode in range(4))               # (0 ESDF / 1 TSDF, mode)
QUERY_COMBOS = tuple((i, g, p) for i in (False, True) for g in (False, True) for p in (False, True))
SQRT_HALF = float(F(np.sqrt(0.5)))
IDENT = np.array([1, 0, 0, 0, 0, 0, 0], F)


def _quat_matrix(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _quarter_turn(rng):
    """a rotation by k * 90 deg, k in 1..3, about one axis: components 0, +-1, +-sqrt(1/2) as f32"""
    axis, k = int(rng.integers(0, 3)), int(rng.integers(1, 4))
    q = np.zeros(4)
    if k == 2:
        q[1 + axis] = rng.choice([-1.0, 1.0])
    else:
        q[0] = SQRT_HALF
        q[1 + axis] = SQRT_HALF if k == 1 else -SQRT_HALF
    return q


def draw_pose(rng, kind, centre, vs):
    """[7] f32 (qw,qx,qy,qz, tx,ty,tz): R about `centre` (f64 [3]) plus a shift.  quarter_turn and grid_shift take the
    shift as whole or half voxels and the translation is rounded to f32 once, so for a dyadic voxel size every sample
    point of the projected map falls on a voxel centre or face."""
    vs = float(F(vs))
    if kind == "identity":
        return IDENT.copy()
    if kind == "yaw":
        a = rng.uniform(-np.pi, np.pi)
        q = np.array([np.cos(a / 2), 0, 0, np.sin(a / 2)])
    elif kind == "full":
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
    elif kind == "near_identity":
        r = rng.normal(size=3) * 1e-4
        q = np.array([1.0, *(0.5 * r)])
        q /= np.linalg.norm(q)
    elif kind == "quarter_turn":
        q = _quarter_turn(rng)
    elif kind == "grid_shift":
        q = np.array([1.0, 0, 0, 0])
    else:
        raise ValueError(kind)
    if kind in ("quarter_turn", "grid_shift"):
        shift = rng.integers(-6, 7, 3) * 0.5 * vs
        R = np.round(_quat_matrix(q / np.linalg.norm(q)))            # the exact signed permutation
    else:
        shift = rng.uniform(-1.5, 1.5, 3) * vs * (1e-3 if kind == "near_identity" else 1.0)
        R = _quat_matrix(q / np.linalg.norm(q))
    t = centre + shift - R @ centre
    T = np.array([*q, *t], F)
    assert abs(float(np.dot(T[:4].astype(np.float64), T[:4].astype(np.float64))) - 1.0) <= 1e-4
    return T


def _transform64(T, p):
    q = np.asarray(T[:4], np.float64)
    return p @ _quat_matrix(q / np.linalg.norm(q)).T + np.asarray(T[4:], np.float64)


def plant_edges(rng, d, w, min_weight):
    """the edge classes, in place: d == 0, -0.0, pairs with |sa - sb| < 1e-6; weight == min_weight, == 1e-6f, == 0,
    1e4; a whole block of zero weight"""
    d[rng.random(d.shape) < 0.03] = 0
    tiny = rng.random(d.shape) < 0.03
    d[tiny] = rng.uniform(-4e-7, 4e-7, int(tiny.sum())).astype(F)
    d[rng.random(d.shape) < 0.02] = F(-0.0)
    w[rng.random(w.shape) < 0.03] = 0
    w[rng.random(w.shape) < 0.03] = F(min_weight)
    w[rng.random(w.shape) < 0.01] = F(1e-6)
    w[rng.random(w.shape) < 0.01] = F(1e4)
    if len(w) > 2 and rng.random() < 0.5:
        w[rng.integers(0, len(w))] = 0


def _block_box(rng, lo, dims, density):
    bi = synth.dense_block_index(lo, dims)
    keep = rng.random(len(bi)) < density
    if not keep.any():
        keep[rng.integers(0, len(bi))] = True
    bi = bi[keep]
    return np.ascontiguousarray(bi[rng.permutation(len(bi))], np.int32)        # shuffled slot order


def _values(rng, kind, world, vs, vps, centre):
    """TSDF distance / weight [n][vps^3] of voxels at world positions [n][vps^3][3] (f64)"""
    n, nv = world.shape[:2]
    bs = vs * vps
    if kind == "noise":
        d = (rng.uniform(-3, 3, (n, nv)) * vs).astype(F)
        return d, rng.uniform(0.1, 30, (n, nv)).astype(F)
    p = world.reshape(-1, 3).astype(F)
    c = (centre + rng.uniform(-0.5, 0.5, 3) * bs).astype(F)
    if kind == "ground":
        sdf = synth.sphere_ground_sdf(c, float(rng.uniform(0.4, 1.0) * bs), float(c[2] - rng.uniform(0.2, 0.8) * bs))
    else:
        sdf = synth.sphere_sdf(c, float(rng.uniform(0.5, 1.4) * bs))
    d = sdf(p).reshape(n, nv).astype(F)
    d = (d + rng.normal(0, 0.02 * vs, d.shape)).astype(F)
    if kind == "truncated":
        trunc = F(3 * vs)
        w = np.where(np.abs(d) <= F(2) * trunc, F(10), F(0)).astype(F)
        return np.clip(d, -trunc, trunc).astype(F), w
    return d, rng.uniform(0.5, 20, (n, nv)).astype(F)


def _submap(vs, vps, bi, d, w):
    return types.SimpleNamespace(voxel_size=float(F(vs)), vps=int(vps), block_index=bi, tsdf_distance=d, tsdf_weight=w)


def draw(seed):
    rng = np.random.default_rng(seed)
    vps = int(rng.choice([8, 16]))
    vs = float(F(VOXEL_SIZES[seed % len(VOXEL_SIZES)]))
    bs = float(F(F(vps) * F(vs)))
    min_weight = MIN_WEIGHTS[(seed + seed // 4) % len(MIN_WEIGHTS)]
    offset = rng.integers(-40, 41, 3) * (rng.random(3) < 0.85)              # (some axes stay at the origin)
    centre = (offset + 1.0) * bs
    n_sub = int(rng.integers(1, 7))
    first_kind = POSE_KINDS[(seed + seed // 6) % len(POSE_KINDS)]
    subs, poses, pose_kinds, value_kinds, shapes = [], [], [], [], []
    for s in range(n_sub):
        shape = SHAPE_KINDS[int(rng.choice(3, p=[0.7, 0.15, 0.15]))]
        if shape == "one_block":
            dims = np.ones(3, np.int64)
        elif shape == "slab":
            dims = np.ones(3, np.int64)
            dims[rng.integers(0, 3)] = rng.integers(2, 5)
        else:
            dims = rng.integers(1, 5, 3)
        lo = offset + rng.integers(-1, 2, 3) - (dims - 2) // 2
        bi = _block_box(rng, lo, dims, rng.uniform(0.3, 1.0))
        kind = first_kind if s == 0 else POSE_KINDS[int(rng.integers(0, len(POSE_KINDS)))]
        T = draw_pose(rng, kind, centre, vs)
        vkind = VALUE_KINDS[(seed + s) % len(VALUE_KINDS)]
        world = _transform64(T, synth.voxel_centres(vs, vps, bi).astype(np.float64))
        d, w = _values(rng, vkind, world, vs, vps, centre)
        plant_edges(rng, d, w, min_weight)
        subs.append(_submap(vs, vps, bi, d, w))
        poses.append(T)
        pose_kinds.append(kind)
        value_kinds.append(vkind)
        shapes.append(shape)
    poses = np.stack(poses).astype(F)
    # a layer that already holds data (with colours), partly under the submaps
    base_bi = _block_box(rng, offset + rng.integers(-1, 1, 3), rng.integers(1, 4, 3), rng.uniform(0.4, 1.0))
    nv = vps ** 3
    base_d = (rng.uniform(-3, 3, (len(base_bi), nv)) * vs).astype(F)
    base_w = rng.uniform(0, 8, (len(base_bi), nv)).astype(F)
    base_w[rng.random(base_w.shape) < 0.2] = 0
    base_rgba = rng.integers(0, 256, (len(base_bi), nv, 4), dtype=np.uint8)
    # the separated mesh's array: every submap, shuffled; every third seed one entry twice (same submap, same pose)
    order = [int(i) for i in rng.permutation(n_sub)]
    duplicate = seed % 3 == 0
    if duplicate:
        order.insert(int(rng.integers(0, len(order) + 1)), order[int(rng.integers(0, len(order)))])
    colors = rng.integers(0, 256, (n_sub, 4), dtype=np.uint8)
    # weld thresholds: all six kinds per seed, rotating over the meshes they are used on
    extent = float(np.abs(centre).max() + 8 * bs)
    thresholds = []
    for i in range(len(THRESHOLD_KINDS)):
        kind = THRESHOLD_KINDS[(seed + i) % len(THRESHOLD_KINDS)]
        value = {"default": 1e-10, "half_voxel": float(F(0.5) * F(vs)), "voxel": vs, "block": bs, "extent": 4 * extent,
                 "log_uniform": 10.0 ** rng.uniform(-20, 1)}[kind]
        thresholds.append((kind, F(value)))
    evals = [EVAL_COMBOS[(2 * seed + i) % 8] for i in range(2)]
    queries = [QUERY_COMBOS[(3 * seed + i) % 8] + (("esdf", "tsdf")[(seed + i) % 2],) for i in range(3)]
    query_kind = first_kind if first_kind != "identity" else "quarter_turn"
    query_pose = draw_pose(rng, query_kind, centre, vs)
    transform_pose = draw_pose(rng, POSE_KINDS[(seed + seed // 6 + 1 + seed % 5) % len(POSE_KINDS)], centre, vs)
    drawn = {"voxel_size": {vs}, "vps": {vps}, "min_weight": {min_weight}, "pose_kind": set(pose_kinds) | {query_kind},
             "value_kind": set(value_kinds), "shape": set(shapes), "threshold_kind": {k for k, _ in thresholds},
             "eval": set(evals), "query": {q[:3] for q in queries}, "query_layer": {q[3] for q in queries},
             "duplicate_entry": {duplicate}, "n_submaps": {n_sub}, "offset_sign": {int(np.sign(o)) for o in offset}}
    return types.SimpleNamespace(seed=seed, vps=vps, voxel_size=vs, block_size=bs, min_weight=min_weight, offset=offset,
                                 centre=centre, subs=subs, poses=poses, pose_kinds=pose_kinds, value_kinds=value_kinds,
                                 shapes=shapes, base=(base_bi, base_d, base_w, base_rgba), sep_order=order, colors=colors,
                                 thresholds=thresholds, evals=evals, queries=queries, query_pose=query_pose,
                                 transform_pose=transform_pose, extent=extent, drawn=drawn, rng=rng)


def describe(sc):
    """the drawn configuration in one line, for a mismatch report"""
    return (f"seed {sc.seed}: vps {sc.vps} voxel_size {sc.voxel_size!r} min_weight {sc.min_weight} offset "
            f"{sc.offset.tolist()} submaps {[(len(s.block_index), k, v, sh) for s, k, v, sh in zip(sc.subs, sc.pose_kinds, sc.value_kinds, sc.shapes)]} "
            f"base {len(sc.base[0])} sep_order {sc.sep_order} thresholds {[(k, float(v)) for k, v in sc.thresholds]} "
            f"evals {sc.evals} queries {sc.queries}")


def query_points(rng, layer, n, pose=None):
    """test_map_query_gpu._points' mixture over `layer`'s blocks (inside, outside, on block faces, on voxel centres /
    faces) in the submap frame; with a pose the same points seen from frame Q (x = T p, f32), the grid points among
    them: voxel centres and faces seen through the pose."""
    from tests import projected_map_ref as pm
    vs, bs = F(layer.voxel_size), F(layer.voxel_size * layer.vps)
    bi = np.asarray(layer.block_index)
    lo = bi.min(0) * bs
    hi = (bi.max(0) + 1) * bs
    inside = rng.uniform(lo, hi, (n, 3)).astype(F)
    outside = rng.uniform(lo - 2 * bs, hi + 2 * bs, (n // 4, 3)).astype(F)
    faces = rng.uniform(lo, hi, (n // 4, 3)).astype(F)
    ax = rng.integers(0, 3, len(faces))
    faces[np.arange(len(faces)), ax] = (np.round(faces[np.arange(len(faces)), ax] / bs) * bs).astype(F)
    m = n // 2
    grid = ((np.floor(rng.uniform(lo, hi, (m, 3)) / vs) + rng.choice([0.0, 0.5], (m, 3))).astype(F) * vs).astype(F)
    p = np.concatenate([inside, outside, faces, grid]).astype(F)
    if pose is not None:
        p = pm.transform(pose[:4], pose[4:], p)
    return p


def eval_partner(rng, sm, vs, vps):
    """a second submap for the evaluation: a part of sm's blocks plus blocks of its own, shuffled; its values are sm's
    plus noise of 1e-6 .. 1e-1 (the squared errors span binades), with d == 0 and -0.0, weight == 1e-6f and unobserved
    ESDF voxels planted.  sm: SubmapData (the downloaded layers)."""
    bi = np.asarray(sm.block_index)
    n, nv = len(bi), vps ** 3
    keep = rng.random(n) < rng.uniform(0.4, 0.9)
    if n and not keep.any():
        keep[rng.integers(0, n)] = True
    lo = bi.min(0) if n else np.zeros(3, np.int64)
    have = {tuple(b) for b in bi.tolist()}
    extra = [b for b in synth.dense_block_index(lo - 1, (3, 3, 2)).tolist() if tuple(b) not in have][:int(rng.integers(1, 5))]
    pbi = np.concatenate([bi[keep], np.array(extra, np.int32).reshape(-1, 3)]).astype(np.int32)
    src = np.concatenate([np.flatnonzero(keep), np.full(len(extra), -1, np.int64)])
    perm = rng.permutation(len(pbi))
    pbi, src = pbi[perm], src[perm]

    def noisy(a, fresh):
        out = fresh.astype(F)
        got = src >= 0
        noise = rng.normal(0, 1, (int(got.sum()), nv)) * 10.0 ** rng.uniform(-6, -1, (int(got.sum()), 1))
        out[got] = (a[src[got]] + noise).astype(F)
        return out

    m = len(pbi)
    td = noisy(sm.tsdf_distance, rng.uniform(-0.3, 0.3, (m, nv)))
    ed = noisy(sm.esdf_distance, rng.uniform(-1, 2, (m, nv)))
    tw = rng.uniform(0, 5, (m, nv)).astype(F)
    eo = (rng.random((m, nv)) < 0.85).astype(np.uint8)
    for d in (td, ed):
        d[rng.random(d.shape) < 0.02] = 0
        d[rng.random(d.shape) < 0.02] = F(-0.0)
    tw[rng.random(tw.shape) < 0.1] = 0
    tw[rng.random(tw.shape) < 0.02] = F(1e-6)
    return synth.SubmapData(float(F(vs)), vps, np.ascontiguousarray(pbi), td, tw, ed, eo, np.zeros(4))


def compare(name, got, want, nan_equal=False):
    """exact comparison of two arrays (or tuples of arrays, None allowed) by their bytes: None when equal, else a
    message with the shapes or the first differing flat indices (of 4-byte words where the item size allows).
    nan_equal (off by default; the layer readers' fuzzer): in a float array a NaN equals a NaN whatever its sign and
    payload -- a kernel and x86 numpy give different default NaNs for inf - inf -- and nothing else changes: -0.0 is
    not +0.0, a NaN is no number."""
    if isinstance(want, (tuple, list)):
        if len(got) != len(want):
            return f"{name}: {len(got)} arrays, want {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            msg = compare(f"{name}[{i}]", g, w, nan_equal)
            if msg:
                return msg
        return None
    if (got is None) != (want is None):
        return f"{name}: got {'None' if got is None else 'an array'}, want {'None' if want is None else 'an array'}"
    if want is None:
        return None
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return f"{name}: shape {g.shape} {g.dtype}, want {w.shape} {w.dtype}"
    if nan_equal and g.dtype.kind == "f":
        word = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]               # one word per number
        a, b = g.reshape(-1).view(word), w.reshape(-1).view(word)
        bad = np.flatnonzero((a != b) & ~(np.isnan(g.reshape(-1)) & np.isnan(w.reshape(-1))))
    else:
        word = np.uint32 if g.dtype.itemsize % 4 == 0 else np.uint8
        a, b = g.reshape(-1).view(word), w.reshape(-1).view(word)
        bad = np.flatnonzero(a != b)
    if len(bad):
        i = int(bad[0])
        return f"{name}: {len(bad)} of {a.size} words differ, first at {bad[:5].tolist()}: got {a[i]:#x} want {b[i]:#x}"
    return None


def compare_layers(name, got, want):
    """two layers {(bx, by, bz): (distance, weight)}"""
    if set(got) != set(want):
        return f"{name}: block sets differ, {sorted(set(got) ^ set(want))[:5]} ({len(got)} got, {len(want)} want)"
    for k in sorted(want):
        msg = compare(f"{name} block {k}", tuple(got[k]), tuple(want[k]))
        if msg:
            return msg
    return None


class Degenerate:
    """the cap on degenerate cases: per product at most one case in five"""

    def __init__(self):
        self.cases, self.degenerate = {}, {}

    def count(self, product, degenerate):
        self.cases[product] = self.cases.get(product, 0) + 1
        self.degenerate[product] = self.degenerate.get(product, 0) + bool(degenerate)

    def exceeded(self):
        return {p: (self.degenerate[p], n) for p, n in self.cases.items() if 5 * self.degenerate[p] > n}
