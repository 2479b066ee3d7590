#!/usr/bin/env python3
"""Differential fuzzing of ONE long-lived registration batch (vgx_reg_batch_*) through random call sequences: the scenes
and sequences of profiles/fuzz_reg_sequence_scene.py (three submaps, four to eight constraints, 14 calls per handle; the
arms, pose classes and ops are listed there).  A batch carries state from call to call -- the launch orders decided at the
first poses of each pass, the dead-tile bits, the pose packs and their staging, the internal [n][45] blocks, the pinned
staging of the host copies, the kept f64 rows with their mirror and flags, the sampling engines -- and every step is
held to what the SAME call gives without that history:
  * rows (evaluate_points, _f64, _blocked, evaluate_rows_f64 + fetch, the drop-in Evaluate and evaluate_visuals): EQUAL to
    oracle.pyoracle.reg_evaluate at the step's poses (f64 equal, f32 equal to the f32 rounding); every caller array is
    pre-filled with NaN;
  * all-points batches: blocks, cost, assembled buffer, scattered array, fetched slices and live counts EQUAL, bit for
    bit, to the same call on a FRESH handle over the same cost functions (made for the step, destroyed after it); the cost
    is also element 0 of the fresh blocks; the fresh blocks within profiles/fuzz_reg.py's bound of the oracle's sums;
  * sampling batches: one orc.Mt19937 per engine, every evaluation of any kind (drop-in included) consumes num_residuals
    draws per constraint in list order, counts / refused calls / fetch / assemble / scatter none: rows equal at the model's
    indices, fused sums and costs within the same bound of the sums at the model's indices; every sequence ends with a
    rows evaluation, so a call that consumed more or fewer draws than the model says is caught;
  * a refused call (n_nodes one too small for each kind of evaluation; a fetch of a Jacobian block the last rows
    evaluation did not produce; assemble / scatter_normal(NULL) while the internal array holds no blocks) returns
    VGX_ERR_INVALID and changes nothing: right after it a fetch, an assemble of the last internal blocks and a rows
    evaluation give what they would have given without it;
  * launch_order is -1 until the pass's first evaluation and never changes afterwards.
A mismatch prints the seed, the step, the op and the poses.  The summary line counts steps, evaluations, refused calls
and, per pass, the seeds whose launch order came out grouped (1) / constraint-major (0).
KEEP_GOING=1 reports the first mismatch of every seed instead of stopping at the first seed that has one.
    SEEDS=240 FIRST=1000 python profiles/fuzz_reg_sequences.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
NORMAL = 45


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def equal(a, b):
    """as numbers (profiles/fuzz_reg.py's comparison of rows): a NaN equals nothing, -0.0 equals 0.0"""
    return a.shape == b.shape and np.array_equal(a, b)


def differ(got, want):
    """where two row arrays first differ, for the report"""
    if got.shape != want.shape:
        return f"shapes {got.shape} {want.shape}"
    bad = np.argwhere(~(got == want))
    return f"{len(bad)} of {got.size} entries differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"


class Failure(Exception):
    pass


def need(cond, *what):
    if not cond:
        raise Failure(" ".join(str(w) for w in what)[:600])


class Runner:
    """one scene on the GPU: the long-lived batch, the model of what it holds, one method per op"""

    def __init__(self, capi, ctx, sc, SS):
        import torch
        self.torch, self.capi, self.ctx, self.sc, self.SS = torch, capi, ctx, sc, SS
        self.model = SS.Model(sc)
        self.n = len(sc.pairs)
        self.handles = []
        self.gs = []
        for k, (sm, (xyz, dist, w)) in enumerate(zip(sc.submaps, sc.points)):
            g = capi.Submap(ctx, k, sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight, sm.esdf_distance, sm.esdf_observed)
            self.handles.append(g)
            g.set_points(capi.POINTS_VOXELS, xyz, dist, w, capi.POINTS_SORT_MORTON if sc.sort_morton[k] else capi.POINTS_KEEP_ORDER)
            self.gs.append(g)
        kw = dict(registration_point_type=capi.POINTS_VOXELS, use_esdf_distance=sc.use_esdf, no_correspondence_cost=sc.no_correspondence_cost)
        if sc.sampling:
            kw.update(sampling_ratio=sc.ratio, sampler_seed=SS.PRIVATE_SEED if sc.private else 0)
        self.cfg = capi.default_config(**kw)
        self.cfs = []
        for c, (a, b) in enumerate(sc.pairs):
            cf = capi.RegistrationCostFunction(ctx, self.gs[a], self.gs[b], self.cfg)
            self.handles.append(cf)
            self.cfs.append(cf)
            need(cf.num_residuals() == sc.residuals[c], "num_residuals", c, cf.num_residuals(), sc.residuals[c])
        self.batch = self.new_batch()
        self.handles.append(self.batch)
        self.visuals = capi.RegVisuals(ctx)
        self.handles.append(self.visuals)
        self.ro = self.batch.row_offsets()
        self.R = int(self.ro[-1])
        self.gi = np.arange(self.n) if sc.global_index is None else np.array(sc.global_index)
        # the model of the handle
        self.internal = dict(state="none")           # "blocks": poses, blocks [n][45] as the host saw them
        self.rows = None                             # dict(want, expect: per constraint (r, jo, je) f64)
        self.caller = {}                             # step -> dict(tensor, poses, blocks)
        self.ran = [False, False]                    # fused pass, materialising pass
        self.order = [None, None]
        self.tally = dict(steps=0, evaluations=0, refused=0)

    def new_batch(self):
        return self.capi.RegistrationBatch(self.ctx, self.cfs, self.sc.pairs, self.sc.global_index, self.sc.n_global)

    def destroy(self):
        for h in reversed(self.handles):
            h.destroy()

    # -- helpers
    def nan(self, shape, dtype):
        t = self.torch.full(shape, float("nan"), dtype=dtype, device="cuda:0")
        self.torch.cuda.synchronize()
        return t

    def host(self, t):
        self.ctx.synchronize()
        return t.cpu().numpy()

    def fresh(self):
        """a batch handle without history over the same cost functions (all-points scenes; a count on any scene)"""
        return self.new_batch()

    def evaluation(self, poses):
        """the oracle's rows of one evaluation of the whole batch (consumes the model's draws)"""
        self.tally["evaluations"] += 1
        return self.model.evaluation(poses)

    def check_order(self, where):
        lo = [self.batch.launch_order(0), self.batch.launch_order(1)]
        for p in range(2):
            if not self.ran[p]:
                need(lo[p] == -1, where, "launch_order", p, "is", lo[p], "before the pass's first evaluation")
            elif self.order[p] is None:
                need(lo[p] in (0, 1), where, "launch_order", p, "is", lo[p], "after the pass's first evaluation")
                self.order[p] = lo[p]
            else:
                need(lo[p] == self.order[p], where, "launch_order", p, "changed from", self.order[p], "to", lo[p])

    def check_status(self, st, ev):
        for c, e in enumerate(ev):
            if e[0]:
                need(st[c] == 0, "status of constraint", c, "is", st[c])

    def check_rows(self, what, ev, r, jo, je, rounding):
        """device rows [R], [R][4], [R][4] (None: not asked for) against the oracle's evaluation"""
        for c, (ok, r0, jo0, je0) in enumerate(ev):
            if not ok:
                continue
            s = slice(int(self.ro[c]), int(self.ro[c + 1]))
            for name, got, want in (("residuals", r, r0), ("jac_ref", jo, jo0), ("jac_read", je, je0)):
                if got is not None and not equal(got[s], want.astype(rounding)):
                    raise Failure(f"{what} {name} of constraint {c} differ from the oracle's: {differ(got[s], want.astype(rounding))}")

    def expected_fused(self, blocks, poses):
        """an all-points scene's assembled buffers of `blocks` come from a fresh handle that evaluated at `poses`"""
        fresh = self.fresh()
        try:
            _, fb = fresh.evaluate_normal(poses)
            need(same(fb, blocks), "the blocks held by the model are not a fresh handle's at their poses")
            out = {}
            for n_nodes in (3, 5):
                buf = self.nan((int(self.capi.load().vgx_reg_fused_size(n_nodes, self.sc.n_global)),), self.torch.float64)
                fresh.assemble(n_nodes, buf.data_ptr())
                out[n_nodes] = self.host(buf)
            return out
        finally:
            fresh.destroy()

    def assembled(self, n_nodes, d_normal):
        buf = self.nan((int(self.capi.load().vgx_reg_fused_size(n_nodes, self.sc.n_global)),), self.torch.float64)
        self.batch.assemble(n_nodes, buf.data_ptr(), d_normal=d_normal)
        return self.host(buf)

    def check_assemble(self, where, source, d_normal, n_nodes):
        """source: the model's dict(poses, blocks) of the array that d_normal (None: the internal one) names"""
        got = self.assembled(n_nodes, d_normal)
        if not self.sc.sampling:
            if "fused" not in source:
                source["fused"] = self.expected_fused(source["blocks"], source["poses"])
            want = source["fused"][n_nodes]
        else:   # no second handle may draw: the same blocks, uploaded to an array of the caller's, through the same handle
            up = self.torch.tensor(source["blocks"], dtype=self.torch.float64, device="cuda:0")
            self.torch.cuda.synchronize()
            want = self.assembled(n_nodes, up.data_ptr())
        need(same(got, want), where, "assembled buffer differs from that of the same blocks without the history")

    def scattered(self, d_normal):
        out = self.nan((self.sc.n_global, NORMAL), self.torch.float64)
        self.batch.scatter_normal(out.data_ptr(), d_normal=d_normal)
        return self.host(out)

    def check_scatter(self, where, source, d_normal):
        got = self.scattered(d_normal)
        want = np.zeros((self.sc.n_global, NORMAL))
        want[self.gi] = source["blocks"]
        need(same(got, want), where, "scattered array differs from the blocks at rows global_index")

    def check_fetch(self, where, c, want):
        r, jo, je = self.batch.fetch_rows_f64(c, self.sc.residuals[c], *want)
        ok, r0, jo0, je0 = self.rows["expect"][c]
        if ok:
            for name, got, want0 in (("residuals", r, r0), ("jac_ref", jo, jo0), ("jac_read", je, je0)):
                if got is not None and not equal(got, want0):
                    raise Failure(f"{where} fetched {name} of constraint {c} differ from the oracle's: {differ(got, want0)}")
        return r, jo, je

    def refused(self, call, *words):
        try:
            call()
        except self.capi.VgxError as e:
            need(e.code == self.capi.ERR_INVALID, "refused with", e.code, "not VGX_ERR_INVALID")
            need(all(w in str(e) for w in words), "the refusal's message does not name the cause:", e)
            self.tally["refused"] += 1
            return
        raise Failure("the call was not refused")

    # -- the ops
    def op_points(self, st, dtype=None, what="evaluate_points"):
        t = self.torch
        dtype = dtype or t.float32
        jac = st.get("jac", (True, True))
        tr, tjo, tje = self.nan((self.R,), dtype), self.nan((self.R, 4), dtype) if jac[0] else None, self.nan((self.R, 4), dtype) if jac[1] else None
        call = self.batch.evaluate_points if dtype == t.float32 else self.batch.evaluate_points_f64
        status = call(st["poses"], tr.data_ptr(), tjo.data_ptr() if jac[0] else 0, tje.data_ptr() if jac[1] else 0)
        self.ran[1] = True
        ev = self.evaluation(st["poses"])
        self.check_status(status, ev)
        self.check_rows(what, ev, self.host(tr), self.host(tjo) if jac[0] else None, self.host(tje) if jac[1] else None,
                        F if dtype == t.float32 else np.float64)

    def op_points_f64(self, st):
        self.op_points(st, self.torch.float64, "evaluate_points_f64")

    def op_points_blocked(self, st):
        nbytes, rows, first = self.batch.blocked_layout()
        blocks = self.nan((nbytes // 4,), self.torch.float32)
        status = self.batch.evaluate_points_blocked(st["poses"], blocks.data_ptr())
        self.ran[1] = True
        ev = self.evaluation(st["poses"])
        self.check_status(status, ev)
        B = self.host(blocks).reshape(-1, 9 * rows)
        r, jo, je = np.full(self.R, np.nan, F), np.full((self.R, 4), np.nan, F), np.full((self.R, 4), np.nan, F)
        for c in range(self.n):
            n = self.sc.residuals[c]
            for k0 in range(0, n, rows):
                blk, m = B[int(first[c]) + k0 // rows], min(rows, n - k0)
                s = slice(int(self.ro[c]) + k0, int(self.ro[c]) + k0 + m)
                r[s], jo[s], je[s] = blk[:m], blk[rows:5 * rows].reshape(rows, 4)[:m], blk[5 * rows:].reshape(rows, 4)[:m]
                need(np.isnan(blk[m:rows]).all() and np.isnan(blk[rows:5 * rows].reshape(rows, 4)[m:]).all(), "blocked: padding written", c)
        self.check_rows("evaluate_points_blocked", ev, r, jo, je, F)

    def op_rows(self, st):
        want = st["want"]
        status = self.batch.evaluate_rows_f64(st["poses"], *want)
        self.ran[1] = True
        ev = self.evaluation(st["poses"])
        self.check_status(status, ev)
        self.rows = dict(want=want, expect=ev, poses=st["poses"])
        for c in range(self.n):
            self.check_fetch("evaluate_rows_f64:", c, want)

    def op_fetch(self, st):
        got = self.check_fetch("fetch_rows_f64:", st["c"], st["want"])
        if not self.sc.sampling:
            fresh = self.fresh()
            try:
                fresh.evaluate_rows_f64(self.rows["poses"], *self.rows["want"])
                ref = fresh.fetch_rows_f64(st["c"], self.sc.residuals[st["c"]], *st["want"])
            finally:
                fresh.destroy()
            need(all((g is None and w is None) or same(g, w) for g, w in zip(got, ref)), "fetched slice differs from a fresh handle's")

    def check_blocks(self, what, blocks, poses):
        """blocks [n][45] of an evaluation at `poses` (consumes the model's draws of one evaluation)"""
        ev = self.evaluation(poses)
        if not self.sc.sampling:
            fresh = self.fresh()
            try:
                _, ref = fresh.evaluate_normal(poses)
            finally:
                fresh.destroy()
            need(same(blocks, ref), what, "blocks differ from a fresh handle's")
        for c, (ok, r0, jo0, je0) in enumerate(ev):
            if ok:
                msg = self.SS.fused_error(blocks[c], *self.SS.sums_and_magnitude(r0, jo0, je0))
                need(msg is None, what, "constraint", c, "against the oracle's sums:", msg)

    def op_normal(self, st):
        if st["into"] == "internal":
            status, host = self.batch.evaluate_normal(st["poses"], None, to_host=st["host"])
            self.ran[0] = True
            self.internal = dict(state="blocks", poses=st["poses"])
            blocks = self.scattered(None)[self.gi]
            tensor = None
        else:
            tensor = self.nan((self.n, NORMAL), self.torch.float64)
            status, host = self.batch.evaluate_normal(st["poses"], tensor.data_ptr(), to_host=st["host"])
            self.ran[0] = True
            blocks = self.host(tensor)
        need(host is None or same(host, blocks), "evaluate_normal: normal_host differs from the device blocks")
        self.check_blocks("evaluate_normal:", blocks, st["poses"])
        if tensor is None:
            self.internal["blocks"] = blocks
        else:
            self.caller[st["index"]] = dict(tensor=tensor, poses=st["poses"], blocks=blocks)

    def op_cost(self, st):
        if st["into"] == "internal":
            status, cost = self.batch.evaluate_cost(st["poses"], None, to_host=True)
            self.ran[0] = True
            self.internal = dict(state="none")
        else:
            tensor = self.nan((self.n,), self.torch.float64)
            host_too = bool(st["index"] % 2)
            status, host = self.batch.evaluate_cost(st["poses"], tensor.data_ptr(), to_host=host_too)
            self.ran[0] = True
            cost = self.host(tensor)
            need(host is None or same(host, cost), "evaluate_cost: cost_host differs from the device costs")
        ev = self.evaluation(st["poses"])
        if not self.sc.sampling:
            fresh = self.fresh()
            try:
                _, ref = fresh.evaluate_cost(st["poses"])
                _, blocks = fresh.evaluate_normal(st["poses"])
            finally:
                fresh.destroy()
            need(same(cost, ref), "evaluate_cost: costs differ from a fresh handle's")
            need(same(cost, np.ascontiguousarray(blocks[:, 0])), "evaluate_cost: not element 0 of the blocks at the same poses")
        for c, (ok, r0, jo0, je0) in enumerate(ev):
            if ok:
                want = float(r0 @ r0)
                need(abs(cost[c] - want) <= 2e-6 * want, "evaluate_cost: constraint", c, cost[c], "against the oracle's", want)

    def source(self, st):
        if st["src"] == "internal":
            need(self.internal["state"] == "blocks", "the generator listed an assembly of blocks the model does not hold")
            return self.internal, None
        return self.caller[st["src"]], self.caller[st["src"]]["tensor"].data_ptr()

    def op_assemble(self, st):
        source, d_normal = self.source(st)
        self.check_assemble("assemble:", source, d_normal, 3 + 2 * (st["index"] % 2))

    def op_scatter(self, st):
        source, d_normal = self.source(st)
        self.check_scatter("scatter_normal:", source, d_normal)
        if d_normal is not None:
            need(same(self.host(source["tensor"]), source["blocks"]), "scatter_normal: the caller's blocks changed")

    def op_count_live(self, st, each=False):
        fresh = self.fresh()
        try:
            if each:
                got, want = self.batch.count_live_each(st["poses"]), fresh.count_live_each(st["poses"])
                need(np.array_equal(got, want), "count_live_each", got, "fresh handle", want)
            else:
                got, want = self.batch.count_live(st["poses"], unique=True), fresh.count_live(st["poses"], unique=True)
                need(got == want, "count_live", got, "fresh handle", want)
        finally:
            fresh.destroy()
        if st["cls"] == "far" and self.sc.no_correspondence_cost == 0.0 and not self.sc.sampling:
            need(not np.any(got if each else got[0]), "live residuals at poses where every chunk is culled:", got)

    def op_count_live_each(self, st):
        self.op_count_live(st, each=True)

    def op_dropin(self, st, visuals=False):
        c = st["c"]
        a, b = self.sc.pairs[c]
        n = self.sc.residuals[c]
        r = np.full(n, np.nan)
        jo, je = (np.full((n, 4), np.nan) if st["jac"][0] else None), (np.full((n, 4), np.nan) if st["jac"][1] else None)
        params = [st["poses"][a], st["poses"][b]]
        if visuals:
            ok = self.cfs[c].evaluate_visuals(params, r, [jo, je], self.visuals)
        else:
            ok = self.cfs[c].Evaluate(params, r, [jo, je])
        self.tally["evaluations"] += 1
        ok0, r0, jo0, je0 = self.model.rows(c, st["poses"], self.model.draw(c))
        need(bool(ok) == bool(ok0), "drop-in return value", ok, ok0)
        if ok0:
            for name, got, want0 in (("residuals", r, r0), ("jac_ref", jo, jo0), ("jac_read", je, je0)):
                if got is not None and not equal(got, want0):
                    raise Failure(f"drop-in {name} of constraint {c} differ from the oracle's: {differ(got, want0)}")
            if visuals:
                need(self.visuals.stats() == (n, n if (st["jac"][0] or st["jac"][1]) else 0), "visuals stats", self.visuals.stats())

    def op_visuals(self, st):
        self.op_dropin(st, visuals=True)

    def op_alloc_outputs(self, st):
        r, jo, je, _ = self.batch.alloc_outputs(st["poses"], 2, *st["jac"])
        self.ran[1] = True
        need(r != 0 and (jo != 0) == st["jac"][0] and (je != 0) == st["jac"][1], "alloc_outputs: arrays", r, jo, je)
        self.batch.free_outputs(r, jo, je)
        self.internal = dict(state="unknown")

    def op_solve(self, st):
        capi, P = self.capi, st["poses"]
        pg = capi.PoseGraph(self.ctx, 3, [1, 0, 0])
        try:
            pg.set_registration(self.batch)
            pg.set_edges([capi.pose_graph_edge(a, b, self.sc.true_poses[b][:3] - self.sc.true_poses[a][:3],
                                               self.sc.true_poses[b][3] - self.sc.true_poses[a][3], np.eye(4)) for a, b in ((0, 1), (1, 2))])
            x, summary = pg.optimize(P, max_num_iterations=st["iterations"])
            need(np.isfinite(x).all(), "solve:", summary)
        finally:
            pg.destroy()
        self.ran[0] = True
        self.internal = dict(state="unknown")

    def after_refusal(self, st):
        """what the handle gives right after a refused call: a fetch, an assemble of the last blocks, a rows evaluation"""
        if self.rows is not None:
            self.check_fetch("after the refused call, fetch_rows_f64:", st["index"] % self.n, self.rows["want"])
        if self.internal["state"] == "blocks":
            self.check_assemble("after the refused call, assemble(NULL):", self.internal, None, 3)
        self.op_points(dict(poses=st["poses"], jac=(True, True)), what="after the refused call, evaluate_points")

    def op_refused(self, st):
        kind, t, short = st["op"][len("refused_"):], self.torch, st["poses"][:2]     # n_nodes = 2: node 2 is listed
        if kind in ("points", "points_f64"):
            dtype = t.float32 if kind == "points" else t.float64
            tr, tjo, tje = self.nan((self.R,), dtype), self.nan((self.R, 4), dtype), self.nan((self.R, 4), dtype)
            call = self.batch.evaluate_points if kind == "points" else self.batch.evaluate_points_f64
            self.refused(lambda: call(short, tr.data_ptr(), tjo.data_ptr(), tje.data_ptr()), "n_nodes")
            need(all(np.isnan(self.host(x)).all() for x in (tr, tjo, tje)), "the refused call wrote rows")
        elif kind == "points_blocked":
            blocks = self.nan((self.batch.blocked_layout()[0] // 4,), t.float32)
            self.refused(lambda: self.batch.evaluate_points_blocked(short, blocks.data_ptr()), "n_nodes")
            need(np.isnan(self.host(blocks)).all(), "the refused call wrote rows")
        elif kind == "rows":
            self.refused(lambda: self.batch.evaluate_rows_f64(short, *st["want"]), "n_nodes")
        elif kind == "normal":
            self.refused(lambda: self.batch.evaluate_normal(short, None, to_host=st["host"]), "n_nodes")
        elif kind == "cost":
            self.refused(lambda: self.batch.evaluate_cost(short, None, to_host=True), "n_nodes")
        elif kind == "fetch":
            self.refused(lambda: self.batch.fetch_rows_f64(st["c"], self.sc.residuals[st["c"]], *st["want"]), "Jacobian block")
        elif kind == "assemble":
            need(self.internal["state"] == "none", "the generator listed a refusal the model does not expect")
            buf = self.nan((int(self.capi.load().vgx_reg_fused_size(3, self.sc.n_global)),), t.float64)
            self.refused(lambda: self.batch.assemble(3, buf.data_ptr()), "holds no blocks")
            need(np.isnan(self.host(buf)).all(), "the refused assemble wrote the fused buffer")
        elif kind == "scatter":
            need(self.internal["state"] == "none", "the generator listed a refusal the model does not expect")
            out = self.nan((self.sc.n_global, NORMAL), t.float64)
            self.refused(lambda: self.batch.scatter_normal(out.data_ptr()), "holds no blocks")
            need(np.isnan(self.host(out)).all(), "the refused scatter_normal wrote the array")
        self.after_refusal(st)

    def step(self, k):
        st = dict(self.sc.steps[k], index=k)
        self.check_order(f"before step {k}:")
        if st["op"].startswith("refused_"):
            self.op_refused(st)
        else:
            getattr(self, "op_" + st["op"])(st)
        self.check_order(f"after step {k}:")
        self.tally["steps"] += 1


def run(n_seeds, first, keep_going=False):
    """-> (0 or 1, summary dict); keep_going: report every seed's first mismatch, not the first seed's alone"""
    from profiles import fuzz_reg_sequence_scene as SS
    from voxgraph_amd import capi
    capi.load()
    ctx = capi.Context(0)
    total = dict(seeds=0, steps=0, evaluations=0, refused=0, grouped=[0, 0], not_grouped=[0, 0])
    rc = 0
    for seed in range(first, first + n_seeds):
        sc = SS.draw(seed)
        run_ = None
        k = -1
        try:
            run_ = Runner(capi, ctx, sc, SS)
            for k in range(len(sc.steps)):
                run_.step(k)
            need(all(o in (0, 1) for o in run_.order), "a pass never ran:", run_.order)
        except (Failure, AssertionError, capi.VgxError) as e:
            print("MISMATCH seed", seed, "step", k, "\n ", str(e)[:600], "\n ", SS.describe(sc, k if k >= 0 else None))
            rc = 1
        finally:
            if run_ is not None:
                for key in ("steps", "evaluations", "refused"):
                    total[key] += run_.tally[key]
                for p in range(2):
                    total["grouped"][p] += run_.order[p] == 1
                    total["not_grouped"][p] += run_.order[p] == 0
                run_.destroy()
        if rc and not keep_going:
            break
        total["seeds"] += 1
    ctx.close()
    if rc == 0:
        print("no mismatch:", total["seeds"], "batches,", total["steps"], "steps,", total["evaluations"], "evaluations,", total["refused"],
              "refused calls; launch order grouped / not grouped: fused pass %d / %d, materialising pass %d / %d"
              % (total["grouped"][0], total["not_grouped"][0], total["grouped"][1], total["not_grouped"][1]))
    return rc, total


def main():
    return run(int(os.environ.get("SEEDS", "100")), int(os.environ.get("FIRST", "0")), bool(int(os.environ.get("KEEP_GOING", "0"))))[0]


if __name__ == "__main__":
    sys.exit(main())
