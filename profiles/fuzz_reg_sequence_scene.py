"""The scene and sequence generator of the registration batch's sequence fuzzer (profiles/fuzz_reg_sequences.py) and of
tests/test_fuzz_reg_sequences_cpu.py.  numpy and oracle/ only: importable without a GPU and without the library.

draw(seed) gives one scene -- three submaps, their registration points, four to eight constraints -- and one sequence of
STEPS calls on ONE batch handle, from np.random.default_rng([seed, TAG, attempt]).  What is categorical follows the seed
round robin with a period of PERIOD = 12 seeds, so that a run of 12 consecutive seeds draws every arm, every planted
point count, every refused-call kind in an all-points and in a sampling seed, and a set of fewer than 64 points:

  arm          = ARMS[seed % 4]
                 shared      at least four constraints on one reference point set of > 4096 points (five 1024-point
                             tiles each: 20 tiles in the fused and in the materialising pass, make_xcd_order refuses
                             fewer than 16), the three submaps on one block box, first poses = the poses they were
                             made at: this is the one arm whose launch orders can come out grouped
                 far_first   no_correspondence_cost 0; the first evaluation of each pass at poses where every chunk is
                             culled, the later ones where the submaps overlap
                 near_first  the reverse: first where they overlap, most of the later ones culled
                 sampling    sampling_ratio from RATIOS, shared (sampler_seed 0) or private engines; the first
                             evaluation of each pass at half-out / yaw-near-pi poses by (seed // 4) % 3
  planted      = PLANTED[(seed % 4 + seed // 4) % 4] points in one submap's set
  small set    = seed % 6 == 5: another submap's set has fewer than 64 points
  sharded      = (seed // 4) % 3 == 1: the batch scatters into a longer global list (global_index, n_global = n + 2)
  refused kinds: REFUSED[(3 * (seed // 4) + i) % 9] for i in 0..2

Everything else -- geometry, counts, weights, the other steps -- comes from the generator.  A scene with an empty point
pool is drawn again with attempt + 1 (scene.attempt tells; the suite's seeds need none).

The sequence keeps a model of what the handle holds while it is drawn (which array the internal blocks are in, what the
last rows evaluation produced), so that every call it lists as refused IS one by the header's rules, and every
assemble / scatter / fetch it lists as valid has something defined to read.  A refused step is the refused call followed
by one f32 rows evaluation at the same poses: what the handle gives right after the refusal."""
import dataclasses
import types

import numpy as np

from oracle import pyoracle as orc
from oracle import synth

F = np.float32
TAG = 0x7371
PERIOD = 12
STEPS = 14
ARMS = ("shared", "far_first", "near_first", "sampling")
PLANTED = (1, 511, 1024, 2049)
RATIOS = (0.05, 0.3, 1.0, 2.5)
POSE_CLASSES = ("near", "half_out", "far", "yaw_pi", "previous")
EVAL_KINDS = ("points", "points_f64", "points_blocked", "rows", "normal", "cost")
REFUSED = tuple("refused_" + k for k in EVAL_KINDS) + ("refused_fetch", "refused_assemble", "refused_scatter")
ALL_POINTS_ONLY = ("alloc_outputs", "solve")
OPS = EVAL_KINDS + ("fetch", "assemble", "scatter", "count_live", "count_live_each", "dropin", "visuals") + ALL_POINTS_ONLY + REFUSED
FUSED_PASS = ("normal", "cost")                                  # the ops that run the fused pass's tiles
POINTS_PASS = ("points", "points_f64", "points_blocked", "rows")  # ... the materialising pass's
PRIVATE_SEED = 5489    # a private engine starts where the reference's WeightedSampler does: the reference's own cost
#                        function (one point-set copy per constraint) can then follow every sampling seed
FAR = np.array([1e4, -3e3, 50.0, 1.0])


def arm_of(seed):
    return ARMS[seed % 4]


def first_classes(seed):
    """(pose class of the first fused evaluation, of the first materialising one)"""
    arm = arm_of(seed)
    if arm == "far_first":
        return "far", "far"
    if arm in ("shared", "near_first"):
        return "near", "near"
    return (("half_out", "yaw_pi"), ("yaw_pi", "half_out"), ("half_out", "half_out"))[(seed // 4) % 3]


def refused_kinds(seed):
    return [REFUSED[(3 * (seed // 4) + i) % 9] for i in range(3)]


def num_residuals(ratio, n_points):
    """RegistrationCostFunction's count (registration_cost_function.cpp:36-38: float arithmetic)"""
    return int(n_points) if ratio is None else int(F(ratio) * F(n_points))


def _submaps(rng, arm):
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.05, 0.1, 0.2]))
    dims = tuple(int(x) for x in (rng.integers(2, 4, 3) if vps == 16 else rng.integers(3, 6, 3)))
    if arm == "shared":
        dims = (3, 3, 2) if vps == 16 else (5, 5, 4)            # room for > 4096 distinct points near the surface
    ext = np.array(dims) * vps * vs
    lo = np.array([int(x) for x in rng.integers(-2, 1, 3)])
    c = (lo * vps * vs) + rng.uniform(0.35, 0.65, 3) * ext
    sdf = synth.sphere_ground_sdf(tuple(c), float(rng.uniform(0.25, 0.4) * ext.min()), float(lo[2] * vps * vs + rng.uniform(0.15, 0.35) * ext[2]))
    sms, true = [], []
    for k in range(3):
        scale = 0.1 if arm == "shared" else 1.0
        T = rng.normal(0, 1, 4) * np.array([vs, vs, 0.5 * vs, 0.02]) * (2.0 * scale) * (k > 0)
        bmin = lo if arm == "shared" else lo + rng.integers(-1, 2, 3) * (rng.random(3) < 0.3)
        sm = synth.make_submap(sdf, vs, vps, tuple(int(x) for x in bmin), dims, trunc=3 * vs, pose=tuple(T), esdf_max=10 * vs,
                               drop_empty_blocks=bool(rng.integers(0, 2)) and arm != "shared")
        if arm != "shared" and len(sm.block_index) > 1:          # blocks dropped at random
            keep = rng.random(len(sm.block_index)) < 0.85
            keep[rng.integers(0, len(keep))] = True
            sm = dataclasses.replace(sm, **{f: np.ascontiguousarray(getattr(sm, f)[keep]) for f in
                                            ("block_index", "tsdf_distance", "tsdf_weight", "esdf_distance", "esdf_observed")})
        sms.append(sm)
        true.append(T)
    return vps, vs, ext, sms, np.array(true)


def _points(rng, sm, use_esdf, count, sampling):
    """count points from the submap's relevant voxels (with repeats when the pool is smaller), in pool order"""
    xyz, dist, w = orc.find_relevant_voxels(sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight,
                                            sm.esdf_distance if use_esdf else None, 1.0, 3.0 * sm.voxel_size)
    if len(w) == 0:
        return None
    idx = np.sort(rng.choice(len(w), count, replace=count > len(w)))
    xyz, dist, w = xyz[idx], dist[idx], w[idx]
    if sampling:                                                  # non-uniform weights, some of them zero
        w = (w * rng.uniform(0.0, 1.0, count) * (rng.uniform(size=count) > 0.1)).astype(F)
        if w.sum() <= 0:
            w[0] = 1.0
    return np.ascontiguousarray(xyz), np.ascontiguousarray(dist), np.ascontiguousarray(w)


def _pairs(rng, arm, ref, usable):
    """four to eight (reference, reading) pairs: at least three (shared arm: four) on `ref`, a mirrored pair, node 2 used"""
    others = [k for k in range(3) if k != ref]
    pairs = [(ref, others[0]), (ref, others[1]), (ref, others[int(rng.integers(0, 2))])]
    if arm == "shared":
        pairs.append((ref, others[int(rng.integers(0, 2))]))
    mirrors = [k for k in others if usable[k]]
    pairs.append((mirrors[int(rng.integers(0, len(mirrors)))], ref))
    candidates = [(a, b) for a in range(3) for b in range(3) if a != b and usable[a]]
    for _ in range(int(rng.integers(0, 9 - len(pairs)))):
        pairs.append(candidates[int(rng.integers(0, len(candidates)))])
    order = rng.permutation(len(pairs))
    return [pairs[i] for i in order]


def poses_of(rng, cls, true, vs, ext):
    """[3][4] node poses of one class"""
    P = true + rng.normal(0, 1, (3, 4)) * np.array([vs, vs, 0.5 * vs, 0.02])
    if cls == "half_out":
        k = int(rng.integers(0, 3))
        P[k] += np.array([0.5 * ext[0] * rng.choice([-1, 1]), 0.5 * ext[1] * rng.choice([-1, 1]), 0.0, 0.5 * rng.normal()])
    elif cls == "far":
        P += np.arange(3)[:, None] * FAR
    elif cls == "yaw_pi":
        P[1, 3] += np.pi - 1e-4 * rng.uniform()
        P[2, 3] -= np.pi - 1e-4 * rng.uniform()
    return P


class _Sequence:
    """draws the steps and keeps the model of the handle's state that decides which calls are valid"""

    def __init__(self, rng, seed, sc):
        self.rng, self.seed, self.sc = rng, seed, sc
        self.steps = []
        self.internal = "none"          # "blocks": of an evaluate_normal(NULL); "none": refused; "unknown": after a solve
        self.rows = None                # (want_jac_ref, want_jac_read) of the last rows evaluation
        self.caller_blocks = []         # steps whose evaluate_normal wrote a caller's array
        self.last_cls, self.last_poses = None, None
        self.done_pass = {"fused": False, "points": False}

    # -- poses
    def _later_class(self):
        arm, r = self.sc.arm, self.rng
        if arm == "far_first":
            return str(r.choice(["near", "half_out", "yaw_pi", "previous"], p=[0.4, 0.2, 0.2, 0.2]))
        if arm == "near_first":
            return str(r.choice(["far", "half_out", "yaw_pi", "previous"], p=[0.55, 0.15, 0.15, 0.15]))
        return str(r.choice(POSE_CLASSES, p=[0.3, 0.2, 0.15, 0.15, 0.2]))

    def _poses(self, cls):
        if cls == "previous":
            if self.last_poses is None:
                cls = "near"
            else:
                return cls, self.last_poses.copy()
        return cls, poses_of(self.rng, cls, self.sc.true_poses, self.sc.voxel_size, self.sc.extent)

    def _eval_class(self, op):
        which = "fused" if op in FUSED_PASS else "points" if op in POINTS_PASS else None
        if which and not self.done_pass[which]:
            return first_classes(self.seed)[0 if which == "fused" else 1]
        return self._later_class()

    # -- one step
    def add(self, op, **kw):
        r = self.rng
        st = dict(op=op, cls=None, poses=None)
        kind = op[len("refused_"):] if op.startswith("refused_") else op
        if op in ("refused_fetch", "refused_assemble", "refused_scatter"):
            st["cls"], st["poses"] = self._poses(self._eval_class("points"))   # of the rows evaluation that follows the refusal
            if op == "refused_fetch":
                st["c"] = int(r.integers(0, len(self.sc.pairs)))
                st["want"] = (not self.rows[0], not self.rows[1])          # the block(s) the last rows evaluation lacks
            self._evaluated("points", st)
        elif kind in EVAL_KINDS:
            refused = op.startswith("refused_")
            # a refused call decides no launch order: the evaluation behind it is a first one if none ran before
            st["cls"], st["poses"] = self._poses(self._eval_class("points" if refused else kind))
            if kind in ("points", "points_f64"):
                st["jac"] = ((True, True), (True, False), (False, True), (False, False))[int(r.integers(0, 4))]
            elif kind == "rows":
                st["want"] = kw.get("want") or ((True, True), (True, False), (False, True), (False, False))[int(r.integers(0, 4))]
            elif kind == "normal":
                st["into"] = kw.get("into") or str(r.choice(["internal", "caller"], p=[0.65, 0.35]))
                st["host"] = bool(r.integers(0, 2)) or (self.sc.sampling and st["into"] == "internal")
            elif kind == "cost":
                st["into"] = kw.get("into") or str(r.choice(["internal", "caller"]))
            if refused:
                self._evaluated("points", st)
            else:
                self._evaluated(kind, st)
                if kind == "rows":
                    self.rows = st["want"]
                elif kind == "normal" and st["into"] == "internal":
                    self.internal = "blocks"
                elif kind == "normal":
                    self.caller_blocks.append(len(self.steps))
                elif kind == "cost" and st["into"] == "internal":
                    self.internal = "none"
        elif op == "fetch":
            st["c"] = int(r.integers(0, len(self.sc.pairs)))
            st["want"] = tuple(bool(h and r.integers(0, 2)) for h in self.rows)
        elif op in ("assemble", "scatter"):
            sources = (["internal"] if self.internal == "blocks" else []) + self.caller_blocks[-2:]
            st["src"] = kw.get("src") or sources[int(r.integers(0, len(sources)))]
            st["src"] = st["src"] if st["src"] == "internal" else int(st["src"])
        elif op in ("count_live", "count_live_each"):
            cls = "far" if self.last_cls in (None, "near", "half_out", "yaw_pi") else "near"   # not the last evaluation's
            st["cls"], st["poses"] = self._poses(cls)
        elif op in ("dropin", "visuals"):
            st["c"] = int(r.integers(0, len(self.sc.pairs)))
            st["jac"] = ((True, True), (True, False), (False, True), (False, False))[int(r.integers(0, 4))]
            st["cls"], st["poses"] = self._poses(self._later_class())
            self.last_cls, self.last_poses = st["cls"], st["poses"]
        elif op == "alloc_outputs":
            st["jac"] = ((True, True), (True, False), (False, True))[int(r.integers(0, 3))]
            st["cls"], st["poses"] = self._poses(self._later_class())
            self.internal = "unknown"
            self.done_pass["points"] = True
        elif op == "solve":
            st["cls"], st["poses"] = self._poses("near")
            st["iterations"] = int(r.integers(1, 4))
            self.internal = "unknown"
            self.done_pass["fused"] = True
        self.steps.append(st)

    def _evaluated(self, kind, st):
        self.done_pass["fused" if kind in FUSED_PASS else "points"] = True
        self.last_cls, self.last_poses = st["cls"], st["poses"]

    # -- what a mandatory step needs in front of it
    def prerequisite(self, op):
        if op == "refused_fetch" and (self.rows is None or all(self.rows)):
            return ("rows", dict(want=((True, False), (False, True), (False, False))[int(self.rng.integers(0, 3))]))
        if op in ("refused_assemble", "refused_scatter") and self.internal != "none":
            return ("cost", dict(into="internal"))
        return None

    def filler(self):
        r, all_points = self.rng, not self.sc.sampling
        ops = {"points": 2, "points_f64": 2, "points_blocked": 2, "rows": 2.5, "normal": 4, "cost": 3, "count_live": 1.2,
               "count_live_each": 1.5, "dropin": 1.5, "visuals": 1.5}
        if self.rows is not None:
            ops["fetch"] = 3
        if self.internal == "blocks" or self.caller_blocks:
            ops["assemble"] = 3
            ops["scatter"] = 3
        if all_points and self.done_pass["fused"] and self.done_pass["points"]:
            ops["alloc_outputs"] = 1.5
            if not self.sc.sharded:
                ops["solve"] = 2.5
        if self.steps and self.steps[-1]["op"] == "count_live_each" and self.internal == "blocks":
            return "assemble", dict(src="internal")                # the blocks a count must not have touched
        if self.steps and self.steps[-1]["op"] == "rows" and r.random() < 0.5:
            return "fetch", {}                                     # straight away; the others come some steps later
        names = list(ops)
        p = np.array([ops[k] for k in names])
        return names[int(r.choice(len(names), p=p / p.sum()))], {}

    def run(self):
        r = self.rng
        firsts = [str(x) for x in r.permutation([str(r.choice(FUSED_PASS)), str(r.choice(POINTS_PASS))])]
        refused = [refused_kinds(self.seed)[i] for i in r.permutation(3)]
        mandatory = firsts + refused
        tail = 1 if self.sc.sampling else 0                        # a sampling sequence ends with a rows evaluation
        while len(self.steps) < STEPS - tail:
            need = sum(2 if m in ("refused_fetch", "refused_assemble", "refused_scatter") else 1 for m in mandatory)
            room = STEPS - tail - len(self.steps) - need
            if mandatory and (len(self.steps) < 2 or room <= 0 or r.random() < 0.3):
                pre = self.prerequisite(mandatory[0])
                if pre:
                    self.add(pre[0], **pre[1])
                    continue
                self.add(mandatory.pop(0))
            else:
                op, kw = self.filler()
                self.add(op, **kw)
        if tail:
            self.add("points")
            self.steps[-1]["jac"] = (True, True)
        return self.steps


def draw(seed):
    arm = arm_of(seed)
    for attempt in range(8):
        rng = np.random.default_rng([seed, TAG, attempt])
        sc = types.SimpleNamespace(seed=seed, arm=arm, attempt=attempt, sampling=arm == "sampling")
        sc.vps, sc.voxel_size, sc.extent, sc.submaps, sc.true_poses = _submaps(rng, arm)
        sc.use_esdf = int(rng.integers(0, 2))
        sc.no_correspondence_cost = 0.0 if arm in ("far_first", "near_first") else float(rng.choice([0.0, 0.25]))
        sc.ratio = float(RATIOS[int(rng.integers(0, 4))]) if sc.sampling else None
        sc.private = bool(rng.integers(0, 2)) if sc.sampling else False
        sc.sharded = (seed // 4) % 3 == 1
        sc.sort_morton = [bool(rng.integers(0, 2)) and sc.sampling for _ in range(3)]
        # point counts: the reference set, the planted one, a third (small on one seed in six)
        sc.reference = int(rng.integers(0, 3))
        planted_at, third = [k for k in rng.permutation(3) if k != sc.reference]
        counts = [0, 0, 0]
        counts[sc.reference] = int(rng.integers(4200, 5000)) if arm == "shared" else int(rng.integers(1500, 5000))
        counts[planted_at] = PLANTED[(seed % 4 + seed // 4) % 4]
        counts[third] = int(rng.integers(1, 64)) if seed % 6 == 5 else int(rng.integers(1500, 5000))
        sc.counts, sc.planted_at, sc.small_at = counts, int(planted_at), (int(third) if seed % 6 == 5 else None)
        sc.points = [_points(rng, sm, sc.use_esdf, counts[k], sc.sampling) for k, sm in enumerate(sc.submaps)]
        if any(p is None for p in sc.points):
            continue
        usable = [num_residuals(sc.ratio, c) > 0 for c in counts]
        if not usable[sc.reference] or not any(usable[k] for k in range(3) if k != sc.reference):
            continue
        sc.pairs = _pairs(rng, arm, sc.reference, usable)
        n = len(sc.pairs)
        sc.n_global = n + 2 if sc.sharded else n
        sc.global_index = [int(x) for x in np.sort(rng.permutation(n + 2)[:n])] if sc.sharded else None
        sc.residuals = [num_residuals(sc.ratio, counts[a]) for a, _ in sc.pairs]
        sc.steps = _Sequence(rng, seed, sc).run()
        return sc
    raise RuntimeError(f"seed {seed}: no scene with points in 8 attempts")


def describe(sc, step=None):
    head = dict(seed=sc.seed, arm=sc.arm, vps=sc.vps, vs=sc.voxel_size, counts=sc.counts, pairs=sc.pairs, esdf=sc.use_esdf,
                nc=sc.no_correspondence_cost, ratio=sc.ratio, private=sc.private, sharded=sc.sharded)
    if step is None:
        return str(head)
    st = sc.steps[step]
    rest = {k: v for k, v in st.items() if k != "poses"}
    poses = None if st["poses"] is None else np.array2string(np.asarray(st["poses"]), precision=17, separator=", ").replace("\n", "")
    return f"{head}\n  step {step}: {rest}\n  poses {poses}"


# ---------------------------------------------------------------------------
# the oracle side: rows of one constraint, the sampling engines, the fused sums
# ---------------------------------------------------------------------------
class Model:
    """the oracle's view of one scene: reading layers, and -- sampling -- one orc.Mt19937 per engine, consumed by
    num_residuals draws per constraint per evaluation in list order"""

    def __init__(self, sc):
        self.sc = sc
        self.layers = []
        for sm in sc.submaps:
            if sc.use_esdf:
                self.layers.append(orc.Layer(sm.voxel_size, sm.vps, sm.block_index, sm.esdf_distance, sm.esdf_observed))
            else:
                self.layers.append(orc.Layer(sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, (sm.tsdf_weight > 0).astype(np.uint8)))
        if sc.sampling:
            self.cums = [np.cumsum(np.asarray(p[2], np.float64)) for p in sc.points]   # WeightedSampler::addItem: one by one, in double
            if sc.private:
                self.engines = [orc.Mt19937(PRIVATE_SEED) for _ in sc.pairs]
            else:
                self.shared = {a: orc.Mt19937(5489) for a in range(3)}

    def engine(self, c):
        return self.engines[c] if self.sc.private else self.shared[self.sc.pairs[c][0]]

    def draw(self, c):
        """the indices constraint c's next Evaluate draws (None: all points)"""
        if not self.sc.sampling:
            return None
        a = self.sc.pairs[c][0]
        eng = self.engine(c)
        return np.array([eng.weighted_draw(self.cums[a]) for _ in range(self.sc.residuals[c])], np.int64)

    def rows(self, c, poses, idx=None):
        """(ok, r, jac_ref, jac_read) of constraint c at node poses [3][4]"""
        a, b = self.sc.pairs[c]
        xyz, dist, w = self.sc.points[a]
        return orc.reg_evaluate(self.layers[b], xyz, dist, w, poses[a], poses[b],
                                no_correspondence_cost=self.sc.no_correspondence_cost, sample_idx=idx)

    def evaluation(self, poses):
        """one evaluation of the whole batch: rows per constraint in list order (this is what consumes the draws)"""
        return [self.rows(c, poses, self.draw(c)) for c in range(len(self.sc.pairs))]


def sums_and_magnitude(r, jo, je):
    """the 45 sums [cost, J^T r (8), upper J^T J (36)] of one constraint's rows and the magnitude of their terms"""
    J = np.concatenate([jo, je], axis=1)
    want = np.r_[float(r @ r), J.T @ r, (J.T @ J)[np.triu_indices(8)]]
    mag = np.r_[float(r @ r), np.abs(J).T @ np.abs(r), (np.abs(J).T @ np.abs(J))[np.triu_indices(8)]]
    return want, mag


def fused_error(block, want, mag):
    """-> None, or what breaks profiles/fuzz_reg.py's bound: each part (cost, J^T r, J^T J) within 2e-6 of its largest
    entry or 5e-7 of the terms' magnitude"""
    for lo, hi in ((0, 1), (1, 9), (9, 45)):
        scale = np.abs(want[lo:hi]).max()
        if scale > 0:
            err = np.abs(block[lo:hi] - want[lo:hi]).max() / scale
            err_mag = (np.abs(block[lo:hi] - want[lo:hi]) / np.maximum(mag[lo:hi], 1e-300)).max()
            if not (err <= 2e-6 or err_mag <= 5e-7):
                return f"part {lo}: {err:.3e} of the largest entry, {err_mag:.3e} of the terms' magnitude"
        elif np.abs(block[lo:hi]).max() != 0:
            return f"part {lo}: not zero"
    return None


# ---------------------------------------------------------------------------
# the launch-order decision's documented inputs (make_xcd_order), restated on the host
# ---------------------------------------------------------------------------
CHUNK = 512
TILE = 1024


def chunk_spheres(xyz):
    """bounding spheres {centre, radius} of consecutive 512-point chunks (chunk_bounds_kernel)"""
    out = []
    for s in range(0, len(xyz), CHUNK):
        p = np.asarray(xyz[s:s + CHUNK], np.float64)
        mn, mx = p.min(0), p.max(0)
        out.append(np.r_[0.5 * (mn + mx), np.linalg.norm(0.5 * (mx - mn)) * 1.0001 + 1e-4])
    return np.array(out)


def chunk_live(sc, c, poses):
    """per 512-point chunk of constraint c's reference points: can its sphere touch the reading submap's block box at
    these poses (chunk_outside; culling applies only where no_correspondence_cost == 0)"""
    a, b = sc.pairs[c]
    sph = chunk_spheres(sc.points[a][0])
    if sc.no_correspondence_cost != 0.0:
        return np.ones(len(sph), bool)
    ta, tb = np.asarray(poses[a], np.float64), np.asarray(poses[b], np.float64)
    ca, sa = np.cos(ta[3]), np.sin(ta[3])
    world = np.stack([ca * sph[:, 0] - sa * sph[:, 1] + ta[0], sa * sph[:, 0] + ca * sph[:, 1] + ta[1], sph[:, 2] + ta[2]], 1) - tb[:3]
    cb, sb = np.cos(tb[3]), np.sin(tb[3])
    q = np.stack([cb * world[:, 0] + sb * world[:, 1], -sb * world[:, 0] + cb * world[:, 1], world[:, 2]], 1)
    sm = sc.submaps[b]
    bs = sm.voxel_size * sm.vps
    lo = sm.block_index.min(0) * bs
    hi = (sm.block_index.max(0) + 2) * bs
    rad = (sph[:, 3] + sm.voxel_size)[:, None]
    return ~(((q + rad) < lo) | ((q - rad) > hi)).any(1)


def order_inputs(sc, poses):
    """(loaded, shareable, all points): the points the tiles load under chunk culling, what of them could come out of
    an L2 (per reference set and 1024-point tile everything beyond the heaviest constraint), and every point listed"""
    work = {}
    total = shareable = everything = 0
    for c, (a, _) in enumerate(sc.pairs):
        n = sc.counts[a]
        live = chunk_live(sc, c, poses)
        pts = np.array([min(CHUNK, n - k * CHUNK) for k in range(len(live))]) * live
        per_tile = [int(pts[2 * t:2 * t + 2].sum()) for t in range(-(-n // TILE))]
        work.setdefault(a, []).append(per_tile)
        everything += n
    for tiles in work.values():
        for t in range(max(len(x) for x in tiles)):
            col = [x[t] for x in tiles if t < len(x)]
            total += sum(col)
            shareable += sum(col) - max(col)
    return total, shareable, everything
