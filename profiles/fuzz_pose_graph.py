#!/usr/bin/env python3
"""Differential fuzzing of the pose-graph solvers (vgx_pose_graph.hip, vgx_tile_pattern.h) against their sequential
restatements (tests/pose_graph_ref.py, pose_graph_sparse_ref.py, pose_graph_covariance_ref.py,
pose_graph_sparse_covariance_ref.py) on the scenes of profiles/fuzz_pose_graph_scene.py.  Per seed:
  1. a block matrix: vgx_block_spd_solve (x, every tile, the tile index, the stats) and vgx_dense_spd_solve by their bits,
     the two next to each other as numbers; both _many calls column by column; in one scene in six a bad pivot first
     (refused by both exactly when the restatements refuse), then the clean matrix, so that nothing sticks;
  2. an edges-only graph: the dense solve, the tile-sparse solve under the drawn ordering (history, summary, costs, poses,
     order, structure, the downloaded system), the sparse solve in natural order next to the dense one as numbers;
  3. its covariances at the start poses: dense, sparse under the drawn ordering with its stats, the drawn budget against
     budget 0, sparse in natural order next to dense as numbers; a rank-deficient graph refused exactly when the
     restatement raises, and the handle solving afterwards as before;
  4. registration constraints over one ring of 12 submaps: the assembled system fed with the batch's own fused buffer,
     and a solve of at most 6 iterations in each solver.
"Bits": every bit of every float64.  "Numbers": np.array_equal (the sign of a zero may differ between sparse and dense).
    SEEDS=300 FIRST=1000 python profiles/fuzz_pose_graph.py          (KEEP_GOING=1: go on after a mismatch)"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles import fuzz_pose_graph_scene as PS  # noqa: E402
from tests import pose_graph_covariance_ref as cov  # noqa: E402
from tests import pose_graph_ref as ref  # noqa: E402
from tests import pose_graph_sparse_covariance_ref as scov  # noqa: E402
from tests import pose_graph_sparse_ref as sref  # noqa: E402

KEYS = ("cost", "trial_cost", "gain_ratio", "radius", "step_norm")
FLAGS = ("accepted", "factorization_failed")
STRUCTURE_KEYS = ("n_free_variables", "n_panels", "n_h_tiles", "n_l_tiles", "n_update_triples", "n_launches")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_numbers(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b)


# ---------------------------------------------------------------------------
# the restatements' side: what tests/test_fuzz_pose_graph_cpu.py runs alone
# ---------------------------------------------------------------------------
def factorised(A, ms, B=None):
    """the two restatements on one matrix -> None where both refuse, else dict(x, L tiles, xd, Ld[, X, Xd])"""
    n, stored = ms.n, [t for t in ms.l_tiles if t in ms.h_keys]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)                    # a tiny pivot may overflow the later columns
        try:
            x, L = sref.spd_solve(sref.to_tiles(A, stored), n, ms.l_tiles, ms.b)
        except ref.NotPositiveDefinite:
            x = None
        try:
            xd, Ld = ref.spd_solve(A, ms.b)
        except ref.NotPositiveDefinite:
            xd = None
        if (x is None) != (xd is None):
            raise AssertionError(f"seed {ms.seed}: the sparse restatement {'refuses' if x is None else 'factorises'} where the dense one does not")
        if x is None:
            return None
        out = dict(x=x, L=L, xd=xd, Ld=Ld)
        if B is not None:
            out["X"], out["Xd"] = scov.solve_many(L, n, ms.l_tiles, B), cov.solve_many(Ld, B)
    return out


def matrix_reference(ms):
    """-> (the clean matrix's results, per bad variant None (refused) or its results)"""
    clean = factorised(ms.A, ms, ms.B)
    assert clean is not None, ms.seed                                      # diagonally dominant
    return clean, [factorised(v.A, ms) for v in ms.bad]


def restated_structure(nf, h_keys, l_tiles):
    return dict(n_free_variables=nf, n_panels=(nf + sref.TILE - 1) // sref.TILE, n_h_tiles=len(h_keys), n_l_tiles=len(l_tiles),
                n_update_triples=len(sref.update_triples(l_tiles)), n_launches=sref.launches(l_tiles))


def graph_reference(gs):
    """-> None for a graph without a free node or without an edge, else dict(dense, sparse: (x, summary, history), keep, H0)"""
    if gs.nfree == 0 or not gs.edges:
        return None
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        dense = ref.solve(ref.ZeroRegistration(), gs.n, gs.constant, gs.edges, gs.poses0, **gs.options)
        keep = {}
        sparse = sref.solve(gs.n, gs.constant, gs.edges, gs.poses0, ordering=gs.ordering, given=gs.given, keep=keep, **gs.options)
    P = np.repeat(4 * np.asarray(keep["order"]), 4) + np.tile(np.arange(4), gs.nfree)
    H0 = np.zeros((gs.nf, gs.nf))
    H0[np.ix_(P, P)] = sref.to_dense(keep["H"], gs.nf)                      # ascending node order whatever the order in use
    return dict(dense=dense, sparse=sparse, keep=keep, H0=H0, structure=restated_structure(gs.nf, keep["h_keys"], keep["l_tiles"]))


def covariance_reference(gs):
    """at the start poses -> None (no free node, no edge or no pair), else dict(H, g, dense, sparse: blocks or None where the
    restatement raises, stats at budget 0 and at the drawn budget, place, l_tiles)"""
    if gs.nfree == 0 or not gs.edges or not gs.cov_pairs:
        return None
    H, g = cov.assembled_system(gs.g)
    joined = [(e[0], e[1]) for e in gs.edges]
    order, place, h_keys, l_tiles = scov.structure(gs.n, gs.constant, joined, gs.ordering, gs.given)
    out = dict(H=H, g=g, place=place, l_tiles=l_tiles, order=order, dense=None, sparse=None,
               stats0=scov.expected_stats(gs.nf, l_tiles, place, gs.cov_pairs, 0),
               stats=scov.expected_stats(gs.nf, l_tiles, place, gs.cov_pairs, gs.max_solve_bytes))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        try:
            out["dense"] = cov.covariance_blocks(H, gs.n, gs.constant, gs.cov_pairs)
        except ref.NotPositiveDefinite:
            pass
        try:
            L = scov.factor(scov.permuted_tiles(H, order, h_keys), gs.nf, l_tiles)
            out["sparse"] = scov.covariance_blocks(None, gs.nf, l_tiles, place, gs.cov_pairs, L=L)
        except ref.NotPositiveDefinite:
            pass
    return out


# ---------------------------------------------------------------------------
# comparisons: a message, or None
# ---------------------------------------------------------------------------
def compare_solve(name, got, want, same=same_bits):
    """got: (x, summary, history) of the library; want: (x, summary, history) of a restatement"""
    (x, s, hist), (x0, s0, hist0) = got, want
    if s["termination"] != s0["termination"] or s["num_iterations"] != s0["num_iterations"]:
        return f"{name}: {s['termination']} after {s['num_iterations']}, want {s0['termination']} after {s0['num_iterations']}"
    if len(hist) != len(hist0):
        return f"{name}: history of {len(hist)}, want {len(hist0)}"
    for k in FLAGS:
        if [h[k] for h in hist] != [h[k] for h in hist0]:
            return f"{name}: history {k} {[h[k] for h in hist]}, want {[h[k] for h in hist0]}"
    for k in KEYS:
        if not same([h[k] for h in hist], [h[k] for h in hist0]):
            return f"{name}: history {k} {[h[k] for h in hist]}, want {[h[k] for h in hist0]}"
    if not same([s["initial_cost"], s["final_cost"]], [s0["initial_cost"], s0["final_cost"]]):
        return f"{name}: costs {s['initial_cost']!r} {s['final_cost']!r}, want {s0['initial_cost']!r} {s0['final_cost']!r}"
    if not same(x, x0):
        return f"{name}: poses differ, max {np.abs(np.asarray(x) - np.asarray(x0)).max():.3e}"
    return None


def compare_counts(name, s, hist):
    """the summary's counts against the library's own history"""
    want = dict(num_successful_steps=sum(h["accepted"] for h in hist), num_factorization_failures=sum(h["factorization_failed"] for h in hist),
                num_full_evaluations=1 + sum(h["accepted"] for h in hist), num_cost_evaluations=sum(1 for h in hist if h["trial_cost"] != 0.0))
    bad = {k: (s[k], v) for k, v in want.items() if s[k] != v}
    return f"{name}: summary counts {bad}" if bad else None


def compare_arrays(name, got, want, same=same_bits):
    if same(got, want):
        return None
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape}, want {want.shape}"
    with np.errstate(all="ignore"):
        return f"{name}: {int((bits(got) != bits(want)).sum())} of {got.size} differ, max {np.nanmax(np.abs(got - want)):.3e}"


# ---------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------
class Totals(dict):
    def add(self, **kw):
        for k, v in kw.items():
            self[k] = self.get(k, 0) + v


def _refusal(capi, call):
    """-> the error code of a refused call, or None where it went through"""
    try:
        call()
    except capi.VgxError as e:
        return e.code
    return None


def matrix_arm(capi, ctx, ms, tot):
    clean, bad_results = matrix_reference(ms)
    n, rows = ms.n, ms.rows
    for v, bad in zip(ms.bad, bad_results):
        values = PS.blocks_of(v.A, dict(bi=ms.bi, bj=ms.bj))
        calls = (("block_spd_solve", lambda: capi.block_spd_solve(ctx, rows, ms.bi, ms.bj, values, ms.b)),
                 ("dense_spd_solve", lambda: capi.dense_spd_solve(ctx, v.A, ms.b)),
                 ("block_spd_solve_many", lambda: capi.block_spd_solve_many(ctx, rows, ms.bi, ms.bj, values, ms.B)),
                 ("dense_spd_solve_many", lambda: capi.dense_spd_solve_many(ctx, v.A, ms.B)))
        if bad is None:
            for name, call in calls:
                code = _refusal(capi, call)
                if code != capi.ERR_NOT_POSITIVE_DEFINITE:
                    return f"{name} on the bad pivot ({v.kind}, row {v.row}): status {code}, want VGX_ERR_NOT_POSITIVE_DEFINITE"
            tot.add(refused_factorisations=1)
        else:                                                              # the restatements factorise it: the usual comparisons
            x, _, index, tiles = calls[0][1]()
            xd, Ld = calls[1][1]()
            msg = (compare_arrays("bad-pivot matrix, block x", x, bad["x"]) or compare_arrays("bad-pivot matrix, dense x", xd, bad["xd"])
                   or compare_arrays("bad-pivot matrix, dense L", Ld, bad["Ld"]))
            if msg:
                return msg
    tot.add(refused_matrices=1 if ms.bad else 0)
    # the clean matrix (after a refusal: nothing sticks)
    x, stats, index, tiles = capi.block_spd_solve(ctx, rows, ms.bi, ms.bj, ms.values, ms.b)
    xd, Ld = capi.dense_spd_solve(ctx, ms.A, ms.b)
    if [tuple(t) for t in index.tolist()] != ms.l_tiles:
        return f"block_spd_solve: tile index {index.tolist()}, want {ms.l_tiles}"
    want = restated_structure(n, {t for t in ms.h_keys if t[0] >= t[1]}, ms.l_tiles)    # (here n_h_tiles: the tiles the lower blocks touch)
    if {k: stats[k] for k in STRUCTURE_KEYS} != want:
        return f"block_spd_solve: stats {stats}, want {want}"
    msg = compare_arrays("block_spd_solve x", x, clean["x"])
    for key, T in zip(index.tolist(), tiles):
        msg = msg or compare_arrays(f"block_spd_solve tile {tuple(key)}", T, clean["L"][tuple(key)])
    L = sref.to_dense({(int(i), int(j)): T for (i, j), T in zip(index, tiles)}, n)
    msg = msg or compare_arrays("block L next to dense L", L, Ld, same_numbers) or compare_arrays("block x next to dense x", x, xd, same_numbers)
    msg = msg or compare_arrays("dense_spd_solve L", Ld, clean["Ld"]) or compare_arrays("dense_spd_solve x", xd, clean["xd"])
    if msg:
        return msg
    B = ms.B.copy()
    X = capi.block_spd_solve_many(ctx, rows, ms.bi, ms.bj, ms.values, B, in_place=ms.in_place)
    if ms.in_place and X is not B:
        return "block_spd_solve_many in place returned another array"
    Xd, _ = capi.dense_spd_solve_many(ctx, ms.A, ms.B)
    msg = compare_arrays(f"block_spd_solve_many m {ms.m}", X, clean["X"]) or compare_arrays(f"dense_spd_solve_many m {ms.m}", Xd, clean["Xd"])
    for c in sorted({0, ms.m // 2, ms.m - 1}):                             # column c IS the single solve of column c
        xc, _, _, _ = capi.block_spd_solve(ctx, rows, ms.bi, ms.bj, ms.values, ms.B[:, c].copy(), want_factor=False)
        xdc, _ = capi.dense_spd_solve(ctx, ms.A, ms.B[:, c].copy(), want_factor=False)
        msg = msg or compare_arrays(f"block_spd_solve_many column {c} against the single solve", X[:, c], xc)
        msg = msg or compare_arrays(f"dense_spd_solve_many column {c} against the single solve", Xd[:, c], xdc)
    tot.add(matrices=1, tiles=len(ms.l_tiles), fill_tiles=len(set(ms.l_tiles) - ms.h_keys), rhs_columns=ms.m)
    tot["worst"] = max(tot.get("worst", 0.0), float(np.abs(L - Ld).max()), float(np.abs(x - xd).max()))
    return msg


def _graph(capi, ctx, gs, edges, solver=None, ordering=sref.NATURAL, given=None):
    pg = capi.PoseGraph(ctx, gs.n, gs.constant)
    if solver is not None:
        pg.set_linear_solver(solver, ordering, given)
    pg.set_edges(edges)
    return pg


def _solved(pg, gs):
    x, s = pg.optimize(gs.poses0, **gs.options)
    return x, s, pg.history()


def graph_arm(capi, ctx, gs, tot):
    sparse_code = capi.LINEAR_SOLVER_TILE_SPARSE
    edges = [capi.pose_graph_edge(*e) for e in gs.edges]
    if not gs.edges:                                                       # one node: nothing can join it
        pg = capi.PoseGraph(ctx, gs.n, gs.constant)
        code = _refusal(capi, lambda: pg.optimize(gs.poses0))
        pg.destroy()
        tot.add(degenerate_graphs=1)
        return None if code == capi.ERR_INVALID else f"a graph without constraints: status {code}, want VGX_ERR_INVALID"
    if gs.nfree == 0:                                                      # hand-stated: the restatements have no such case
        for solver in (None, sparse_code):
            pg = _graph(capi, ctx, gs, edges, solver, gs.ordering if solver else sref.NATURAL, gs.given if solver else None)
            x, s, hist = _solved(pg, gs)
            blocks = pg.covariance(gs.poses0, gs.cov_pairs) if solver is None else pg.covariance_sparse(gs.poses0, gs.cov_pairs)[0]
            pg.destroy()
            if s["termination_reason"] != capi.TERMINATION_NO_FREE_NODES or s["num_iterations"] != 0 or hist or not same_bits(x, gs.poses0):
                return f"all nodes constant: {s}, history of {len(hist)}"
            if blocks.any():
                return "all nodes constant: a covariance block that is not zero"
        tot.add(degenerate_graphs=1)
        return None
    want, cw = graph_reference(gs), covariance_reference(gs)
    dense, sparse = _graph(capi, ctx, gs, edges), _graph(capi, ctx, gs, edges, sparse_code, gs.ordering, gs.given)
    natural = sparse if gs.ordering == sref.NATURAL else _graph(capi, ctx, gs, edges, sparse_code)
    try:
        got_d, got_s = _solved(dense, gs), _solved(sparse, gs)
        msg = compare_solve("dense solve", got_d, want["dense"]) or compare_counts("dense solve", got_d[1], got_d[2])
        msg = msg or compare_solve(f"sparse solve, ordering {gs.ordering}", got_s, want["sparse"]) or compare_counts("sparse solve", got_s[1], got_s[2])
        if msg:
            return msg
        if sparse.order().tolist() != list(want["keep"]["order"]):
            return f"order {sparse.order().tolist()}, want {list(want['keep']['order'])}"
        stats = sparse.structure()
        if {k: stats[k] for k in STRUCTURE_KEYS} != want["structure"]:
            return f"structure {stats}, want {want['structure']}"
        Hs, gsys = sparse.download_system()
        Hd, gd = dense.download_system()
        msg = compare_arrays("sparse download_system H", Hs, want["H0"]) or compare_arrays("sparse download_system g", gsys, want["keep"]["g"])
        got_n = got_s if natural is sparse else _solved(natural, gs)
        msg = msg or compare_solve("sparse solve in natural order next to the dense solve", got_n, got_d, same_numbers)
        Hn, gn = natural.download_system()
        msg = msg or compare_arrays("natural-order H next to the dense H", Hn, Hd, same_numbers) or compare_arrays("natural-order g", gn, gd, same_numbers)
        if msg:
            return msg
        hist = got_d[2]
        tot.add(solves=3 if natural is not sparse else 2, iterations=len(hist), accepted=sum(h["accepted"] for h in hist),
                rejected=sum(1 for h in hist if not h["accepted"] and not h["factorization_failed"] and h["trial_cost"] != 0.0),
                graph_tiles=stats["n_l_tiles"], graph_fill_tiles=stats["n_l_tiles"] - (stats["n_h_tiles"] + stats["n_panels"]) // 2)
        tot["worst"] = max(tot.get("worst", 0.0), float(np.abs(got_s[0] - got_d[0]).max()))
        # covariances at the start poses
        if not gs.cov_pairs:
            blocks, stats = sparse.covariance_sparse(gs.poses0, [])
            if blocks.shape != (0, 4, 4) or any(stats.values()) or dense.covariance(gs.poses0, []).shape != (0, 4, 4):
                return f"an empty pair list: {blocks.shape}, {stats}"
            return None
        if (cw["dense"] is None) != (cw["sparse"] is None) and gs.ordering == sref.NATURAL:
            return "the restatements disagree on the rank of H in natural order"
        for name, pg, call, expected in (("covariance", dense, lambda: dense.covariance(gs.poses0, gs.cov_pairs), cw["dense"]),
                                         ("covariance_sparse", sparse, lambda: sparse.covariance_sparse(gs.poses0, gs.cov_pairs), cw["sparse"])):
            if expected is None:
                code = _refusal(capi, call)
                if code != capi.ERR_NOT_POSITIVE_DEFINITE:
                    return f"{name} of a rank-deficient graph: status {code}, want VGX_ERR_NOT_POSITIVE_DEFINITE"
                again = _solved(pg, gs)                                    # the handle afterwards solves as a fresh one does
                msg = compare_solve(f"the solve after the refused {name}", again, got_d if pg is dense else got_s)
                if msg:
                    return msg
                tot.add(refused_covariances=1)
        if cw["dense"] is not None:
            blocks_d = dense.covariance(gs.poses0, gs.cov_pairs)
            Hc, gc = dense.download_system()
            msg = (compare_arrays("covariance", blocks_d, cw["dense"]) or compare_arrays("H after covariance", Hc, cw["H"])
                   or compare_arrays("g after covariance", gc, cw["g"]))
            if msg:
                return msg
        if cw["sparse"] is not None:
            blocks_s, stats0 = sparse.covariance_sparse(gs.poses0, gs.cov_pairs)
            Hc, _ = sparse.download_system()
            blocks_b, stats = sparse.covariance_sparse(gs.poses0, gs.cov_pairs, max_solve_bytes=gs.max_solve_bytes)
            msg = compare_arrays(f"covariance_sparse, ordering {gs.ordering}", blocks_s, cw["sparse"]) or compare_arrays("H after covariance_sparse", Hc, cw["H"])
            msg = msg or compare_arrays(f"covariance_sparse with max_solve_bytes {gs.max_solve_bytes} against budget 0", blocks_b, blocks_s)
            if msg is None and (stats0 != cw["stats0"] or stats != cw["stats"]):
                msg = f"covariance_sparse stats {stats0} / {stats}, want {cw['stats0']} / {cw['stats']}"
            if msg is None and cw["dense"] is not None:
                blocks_n = blocks_s if natural is sparse else natural.covariance_sparse(gs.poses0, gs.cov_pairs)[0]
                msg = compare_arrays("natural-order sparse blocks next to the dense blocks", blocks_n, blocks_d, same_numbers)
                tot["worst"] = max(tot.get("worst", 0.0), float(np.abs(blocks_n - blocks_d).max()))
            if msg:
                return msg
            tot.add(covariance_columns=stats["n_columns"], slabs=stats["n_slabs"], covariance_calls=1)
        return None
    finally:
        for pg in {id(p): p for p in (dense, sparse, natural)}.values():
            pg.destroy()


class RingOf12:
    """the submaps of tests/pose_graph_ref.ring_graph(12), built once; a batch per seed over them"""

    def __init__(self, capi, ctx):
        from tests import helpers as H
        self.capi, self.ctx = capi, ctx
        self.g = ref.ring_graph(PS.RING, seed=0)
        self.submaps = [H.gpu_submap(capi, ctx, sm, i) for i, sm in enumerate(ref.ring_submaps(self.g))]
        for s in self.submaps:
            s.extract_voxel_points()
        self.cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)

    def destroy(self):
        for s in self.submaps:
            s.destroy()


def registration_arm(capi, ctx, ring, rs, tot):
    from tests.test_pose_graph_gpu import GpuRegistration
    cfs = [capi.RegistrationCostFunction(ctx, ring.submaps[a], ring.submaps[b], ring.cfg) for a, b in rs.pairs]
    batch = capi.RegistrationBatch(ctx, cfs, rs.pairs)
    reg = GpuRegistration(capi, ctx, batch, PS.RING, rs.pairs)
    edges = [capi.pose_graph_edge(*e) for e in rs.edges]
    graphs = []

    def graph(solver=None):
        pg = capi.PoseGraph(ctx, PS.RING, rs.constant)
        if solver is not None:
            pg.set_linear_solver(solver, rs.ordering, rs.given)
        pg.set_registration(batch)
        pg.set_edges(edges)
        graphs.append(pg)
        return pg

    try:
        kw = dict(max_solver_time_in_seconds=600.0, initial_trust_region_radius=rs.radius)
        pg = graph()
        x, s = pg.optimize(rs.poses0, max_num_iterations=0)
        Hg, gg = pg.download_system()
        fused, _ = reg.full(rs.poses0)
        terms = [ref.edge_terms(e, rs.poses0[e[0]], rs.poses0[e[1]]) for e in rs.edges]
        H0, g0 = ref.assemble(PS.RING, rs.constant, rs.pairs, fused, rs.edges, terms)
        msg = compare_arrays("assembled H with registration", Hg, H0) or compare_arrays("assembled g with registration", gg, g0)
        if msg is None and not np.abs(np.asarray(fused[1 + 20 * PS.RING:])).max() > 0:
            msg = "no registration constraint contributes"
        if msg:
            return msg
        got = pg.optimize(rs.poses0, max_num_iterations=rs.max_num_iterations, **kw) + (pg.history(),)
        want = ref.solve(reg, PS.RING, rs.constant, rs.edges, rs.poses0, max_num_iterations=rs.max_num_iterations, **kw)
        msg = compare_solve("dense solve with registration", got, want)
        if msg:
            return msg
        sp = graph(capi.LINEAR_SOLVER_TILE_SPARSE)
        got = sp.optimize(rs.poses0, max_num_iterations=rs.max_num_iterations, **kw) + (sp.history(),)
        want = sref.solve(PS.RING, rs.constant, rs.edges, rs.poses0, ordering=rs.ordering, given=rs.given,
                          max_num_iterations=rs.max_num_iterations, registration=reg, **kw)
        tot.add(registration_solves=2, registration_constraints=len(rs.pairs))
        return compare_solve(f"sparse solve with registration, ordering {rs.ordering}", got, want)
    finally:
        for o in graphs + [batch] + cfs:
            o.destroy()


def main():
    from voxgraph_amd import capi
    capi.load()
    import torch
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n_seeds, first = int(os.environ.get("SEEDS", "100")), int(os.environ.get("FIRST", "0"))
    keep_going = os.environ.get("KEEP_GOING", "0") != "0"                   # report every seed that differs, not the first alone
    tot = Totals()
    ring = RingOf12(capi, ctx)
    status = 0
    for seed in range(first, first + n_seeds):
        sc = PS.scene(seed)
        for arm, msg in (("matrix", lambda: matrix_arm(capi, ctx, sc.matrix, tot)), ("graph", lambda: graph_arm(capi, ctx, sc.graph, tot)),
                         ("registration", lambda: registration_arm(capi, ctx, ring, sc.registration, tot))):
            msg = msg()
            if msg:
                print("MISMATCH seed", seed, "arm", arm, "\n ", msg, "\n ", PS.describe(sc))
                status = 1
                break
        if status and not keep_going:
            break
        tot.add(seeds=1)
    ring.destroy()
    ctx.close()
    if status:
        return 1
    degenerate = tot.get("degenerate_graphs", 0) + tot.get("refused_covariances", 0) // 2 + tot.get("refused_matrices", 0)
    print("totals:", dict(tot))
    if 5 * degenerate > 2 * tot["seeds"]:
        print("TOO MANY REFUSED OR DEGENERATE SCENES (more than one in five of the matrix and graph scenes):", degenerate)
        return 1
    print("no mismatch:", tot["seeds"], "seeds,", tot.get("matrices", 0), "matrices,", tot.get("tiles", 0), "tiles,", tot.get("solves", 0), "solves,",
          tot.get("iterations", 0), "iterations, worst |sparse - dense|", tot.get("worst", 0.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
