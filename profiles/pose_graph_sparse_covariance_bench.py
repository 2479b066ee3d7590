"""vgx_pose_graph_covariance_sparse against the dense vgx_pose_graph_covariance on the same graph, in one process, on one
MI355X: the two graphs of profiles/pose_graph_bench.py (config-3 shape: 200 nodes; config-5 shape: 1000 nodes) with the
covariance block of every registration pair, and tests/pose_graph_sparse_ref.long_graph(4200) (edges only, 16796
unknowns, past the dense limit: the sparse call alone) with the block of every edge -- every free node a second node,
so the whole inverse's block columns are solved.  Natural and RCM order, at the start poses.

The calls alternate; 2 warm-ups, then the median of 5.  The split is by difference, as profiles/pose_graph_covariance_bench.py
does it: the evaluation is timed on its own (a solve of zero iterations); a call for the one pair (n, n), n the node at
the LAST position of the order in use, evaluates and factorises like any other but solves four columns over one panel,
so factorisation = that call - evaluation and solves + gather = all pairs - that call.
Usage: python profiles/pose_graph_sparse_covariance_bench.py [--out profiles/pose_graph_sparse_covariance.txt]"""
import argparse
import os
import statistics
import sys
import time

for _name in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_name, "16")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t0


def split(pg, call, poses, pairs, last, warmup, repeats):
    """-> (medians in ms: evaluation, one pair, all pairs; the last result of `call(pairs)`)"""
    rows, out = [], None
    for r in range(warmup + repeats):
        _, t_eval = timed(lambda: pg.optimize(poses, max_num_iterations=0))
        _, t_one = timed(lambda: call([(last, last)]))
        out, t_all = timed(lambda: call(pairs))
        if r >= warmup:
            rows.append((t_eval, t_one, t_all))
    return [statistics.median(row[k] for row in rows) * 1e3 for k in range(3)], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-long", action="store_true")
    a = ap.parse_args()
    import torch
    import pose_graph_bench
    from tests import pose_graph_sparse_ref as sref
    from voxgraph_amd import capi
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lines = []

    def report(text):
        print(text, flush=True)
        lines.append(text)

    scenes = [("config-3 shape", (20, 10), 0), ("config-5 shape", (100, 10), 50)] + ([] if a.skip_long else [("long_graph(4200)", None, 0)])
    for name, grid, loop_every in scenes:
        if grid is not None:
            n, poses, pairs, batch, edges = pose_graph_bench.build(capi, ctx, grid, loop_every)
            constant = None
        else:
            g = sref.long_graph(4200, seed=0)
            n, poses, batch, edges, constant = g["n"], g["poses0"], None, g["edges"], g["constant"]
            pairs = [(e[0], e[1]) for e in edges]
        edge_items = [capi.pose_graph_edge(*e) for e in edges]
        nf = 4 * (n - 1)
        seconds = len({b for a_, b in pairs if a_ > 0 and b > 0})
        report(f"{name}: {n} nodes, {len(pairs)} pairs, {nf} unknowns, {4 * seconds} columns solved, {(nf + 63) // 64} panels")
        dense_blocks = None
        if nf <= 4 * 4096:
            pg = capi.PoseGraph(ctx, n)
            pg.set_registration(batch)
            pg.set_edges(edge_items)
            med, dense_blocks = split(pg, lambda pr: pg.covariance(poses, pr), poses, pairs, n - 1, a.warmup, a.repeats)
            report(f"  dense  vgx_pose_graph_covariance:               {med[2]:9.2f} ms = evaluation {med[0]:7.2f} + factorisation {med[1] - med[0]:8.2f} "
                   f"+ solves and gather {med[2] - med[1]:8.2f}; {3 * ((nf + 63) // 64) - 2} + 4 launches, X {8 * nf * 4 * seconds / 2**20:.0f} MiB")
            pg.destroy()
        else:
            report("  dense  vgx_pose_graph_covariance:               refused (more than 4096 free nodes)")
        for ordering, code in (("natural", capi.ORDER_NATURAL), ("RCM", capi.ORDER_RCM)):
            pg = capi.PoseGraph(ctx, n, constant, linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE, ordering=code)
            if batch is not None:
                pg.set_registration(batch)
            pg.set_edges(edge_items)
            pg.covariance_sparse(poses, pairs[:1])                       # makes the lists: the order is known
            last = int(pg.order()[-1]) + 1                               # node 0 alone is constant: node = free index + 1
            med, (blocks, stats) = split(pg, lambda pr: pg.covariance_sparse(poses, pr), poses, pairs, last, a.warmup, a.repeats)
            st = pg.structure()
            text = (f"  sparse vgx_pose_graph_covariance_sparse {ordering:8s}{med[2]:9.2f} ms = evaluation {med[0]:7.2f} + factorisation {med[1] - med[0]:8.2f} "
                    f"+ solves and gather {med[2] - med[1]:8.2f}; {st['n_h_tiles']} H tiles, {st['n_l_tiles']} L tiles, {stats['n_slabs']} slab(s), "
                    f"{stats['n_launches']} launches, X {stats['solve_bytes'] / 2**20:.0f} MiB")
            if dense_blocks is not None:
                worst = np.abs(blocks - dense_blocks).max() / np.abs(dense_blocks).max()
                text += f"; equal to the dense blocks: {bool(np.array_equal(blocks, dense_blocks))} (largest difference {worst:.2e} of the largest entry)"
            report(text)
            pg.destroy()
        if batch is not None:
            batch.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
