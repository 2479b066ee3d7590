"""vgx_pose_graph_optimize against harness.lm.solve over the same GpuBackend, on one MI355X, in one run.

Two graphs, both sized down in voxels (4 x 4 x 2 blocks of 16^3 per submap) so that a run takes seconds:
  config-3 shape   20 x 10 grid of submaps, bench.py's neighbour pairs (1176) plus odometry along the numbering
  config-5 shape   100 x 10 grid (1000 nodes), odometry, loop closures every 50 nodes
The two solvers alternate; 2 warm-ups, then the median of 5.  Per solve: total seconds, seconds in the registration
evaluations, seconds in the linear algebra, iterations.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of
this script of its own (--only library).  Usage: python profiles/pose_graph_bench.py [--out profiles/pose_graph.txt]

--solvers: the dense linear solver against the tile-sparse one (natural order and RCM) on ONE handle and scene,
alternating, 2 warm-ups and the median of 9: the solve's linear-algebra seconds per iteration (tiles from H, damping,
factorisation, substitutions, H step and the step's copy to the host: one synchronisation), with the structure's launches
per factorisation, tiles and bytes.  Then the sparse solver alone on edges-only paths of 8000 and 20000 nodes
(tests/pose_graph_sparse_ref.long_graph), past the dense limit.  Appends to --out."""
import argparse
import os
import statistics
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(capi, ctx, grid, loop_every):
    import bench
    from tests import pose_graph_ref as ref
    args = types.SimpleNamespace(grid=list(grid), block_dims=[4, 4, 2], voxel_size=0.2, seed=2, pose_sigma=0.1, yaw_sigma=0.02)
    true, poses, pairs = bench.build_graph(args)[:3]
    n = len(true)
    submaps = []
    for k in range(n):
        sm = capi.Submap.synth_city(ctx, k, 0.2, 16, [-2, -2, -1], args.block_dims, 0.6, 2.0, 10.0, true[k], args.seed)
        sm.extract_voxel_points(1.0, 0.3, True)
        sm.release_raw_layers()
        submaps.append(sm)
    cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
    cfs = [capi.RegistrationCostFunction(ctx, submaps[a], submaps[b], cfg) for a, b in pairs]
    batch = capi.RegistrationBatch(ctx, cfs, pairs)
    edges = [ref.relative_edge(k, k + 1, poses[k], poses[k + 1], ref.INFO_ODOMETRY) for k in range(n - 1)]
    if loop_every:
        edges += [ref.relative_edge(k, k - loop_every, true[k], true[k - loop_every], ref.INFO_LOOP_CLOSURE)
                  for k in range(loop_every, n, loop_every)]
    return n, np.asarray(poses, np.float64), [tuple(map(int, p)) for p in pairs], batch, edges


def solver_lines(capi, ctx, name, pg, poses, n_free, repeats, with_dense, **kw):
    """the solvers alternating on one handle -> text lines"""
    modes = ([("dense", capi.LINEAR_SOLVER_DENSE, capi.ORDER_NATURAL)] if with_dense else []) + [
        ("sparse natural", capi.LINEAR_SOLVER_TILE_SPARSE, capi.ORDER_NATURAL), ("sparse rcm", capi.LINEAR_SOLVER_TILE_SPARSE, capi.ORDER_RCM)]
    rows, stats, ends = {m[0]: [] for m in modes}, {}, {}
    for r in range(2 + repeats):
        for label, solver, ordering in modes:
            pg.set_linear_solver(solver, ordering)
            x, s = pg.optimize(poses, max_solver_time_in_seconds=120.0, **kw)
            if solver == capi.LINEAR_SOLVER_TILE_SPARSE:
                stats[label] = pg.structure()
            ends[label] = x
            if r >= 2:
                rows[label].append(s)
    lines = [f"{name}: {n_free} free nodes, {4 * n_free} unknowns; median of {repeats}, the solvers alternating on one handle"]
    for label, _, _ in modes:
        it = rows[label][0]["num_iterations"]
        la = statistics.median(s["linear_algebra_seconds"] for s in rows[label])
        total = statistics.median(s["total_seconds"] for s in rows[label])
        st = stats.get(label)
        panels = (4 * n_free + 63) // 64
        shape = (f"{st['n_launches']} launches per factorisation, {st['n_l_tiles']} L tiles + {st['n_h_tiles']} H tiles, {st['n_update_triples']} "
                 f"triples, {st['bytes'] / 2**20:.1f} MiB" if st else
                 f"{3 * panels - 2} launches per factorisation, {panels * (panels + 1) // 2} lower tiles' worth, {2 * (4 * n_free) ** 2 * 8 / 2**20:.1f} MiB")
        first = ends[modes[0][0]]
        lines.append(f"  {label:15s} {rows[label][0]['termination']:>20} after {it:2d} iterations: total {total * 1e3:9.2f} ms, linear algebra "
                     f"{la * 1e3:9.2f} ms ({la * 1e3 / max(it, 1):8.3f} ms per iteration); {shape}; end poses vs {modes[0][0]} "
                     f"{np.abs(ends[label] - first).max():.2e}")
    return lines


def solvers(capi, ctx, a):
    from tests import pose_graph_sparse_ref as sref
    lines = []
    for name, grid, loop_every in (("config-3 shape", (20, 10), 0), ("config-5 shape", (100, 10), 50)):
        n, poses, pairs, batch, edges = build(capi, ctx, grid, loop_every)
        pg = capi.PoseGraph(ctx, n)
        pg.set_registration(batch)
        pg.set_edges([capi.pose_graph_edge(*e) for e in edges])
        lines += solver_lines(capi, ctx, f"{name} ({len(pairs)} registration constraints, {len(edges)} edges)", pg, poses, n - 1, a.solver_repeats, True)
        pg.destroy()
        batch.destroy()
    for n in (8000, 20000):
        g = sref.long_graph(n, seed=0)
        pg = capi.PoseGraph(ctx, n, g["constant"], linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE)
        pg.set_edges([capi.pose_graph_edge(*e) for e in g["edges"]])
        lines += solver_lines(capi, ctx, f"path of {n} nodes, edges only ({len(g['edges'])} edges)", pg, g["poses0"], n - 1, a.solver_repeats, False,
                              initial_trust_region_radius=1e8, max_num_iterations=4)
        pg.destroy()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solvers", action="store_true", help="dense against tile-sparse on one handle; appends to --out")
    ap.add_argument("--solver-repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("both", "library"), default="both")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from harness import lm
    from harness.backends import GpuBackend
    from tests import pose_graph_ref as ref
    from voxgraph_amd import capi
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lines = []
    if a.solvers:
        text = "\n".join(solvers(capi, ctx, a))
        print(text)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        ctx.close()
        return
    for name, grid, loop_every in (("config-3 shape", (20, 10), 0), ("config-5 shape", (100, 10), 50)):
        n, poses, pairs, batch, edges = build(capi, ctx, grid, loop_every)
        pg = capi.PoseGraph(ctx, n)
        pg.set_registration(batch)
        pg.set_edges([capi.pose_graph_edge(*e) for e in edges])
        backend = GpuBackend(capi, ctx, batch, n)
        lib, har = [], []
        for r in range(a.warmup + a.repeats):
            x, s = pg.optimize(poses, max_solver_time_in_seconds=60.0)
            if a.only == "both":
                xh, sh = lm.solve(lm.Problem(backend, n, pairs, ref.lm_edges(edges)), poses, max_seconds=60.0)
            if r >= a.warmup:
                lib.append(s)
                if a.only == "both":
                    har.append(sh)
        med = lambda rows, k: statistics.median(row[k] for row in rows)
        it = lib[0]["num_iterations"]
        lines.append(f"{name}: {n} nodes, {len(pairs)} registration constraints, {len(edges)} edges, {4 * (n - 1)} unknowns")
        lines.append(f"  library  {lib[0]['termination']:>20} after {it:2d} iterations ({lib[0]['num_full_evaluations']} full + "
                     f"{lib[0]['num_cost_evaluations']} cost-only evaluations): total {med(lib, 'total_seconds') * 1e3:8.2f} ms, "
                     f"registration {med(lib, 'registration_seconds') * 1e3:8.2f} ms, linear algebra {med(lib, 'linear_algebra_seconds') * 1e3:8.2f} ms "
                     f"({med(lib, 'linear_algebra_seconds') * 1e3 / max(it, 1):.2f} ms per iteration)")
        if har:
            dt = np.abs(x[:, :3] - xh[:, :3]).max()
            dyaw = np.rad2deg(np.abs(lm.normalize_angle(x[:, 3] - xh[:, 3])).max())
            lines.append(f"  harness  {har[0]['termination']:>20} after {har[0]['iterations']:2d} iterations ({har[0]['evaluations']} full evaluations"
                         f"): total {med(har, 'seconds') * 1e3:8.2f} ms, registration {med(har, 'backend_seconds') * 1e3:8.2f} ms, host linear algebra "
                         f"{med(har, 'host_linear_algebra_seconds') * 1e3:8.2f} ms")
            lines.append(f"  end poses, library vs harness: {dt:.3e} m, {dyaw:.3e} deg")
        pg.destroy()
        batch.destroy()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
