"""vgx_pose_graph_covariance against the only route to the same numbers without it -- vgx_pose_graph_download_system, a
host LAPACK inverse (numpy.linalg.inv, at most 16 threads) and block extraction -- on one MI355X, in one run.

The two graphs of profiles/pose_graph_bench.py (config-3 shape: 200 nodes, 1176 pairs; config-5 shape: 1000 nodes), the
covariance block of every registration pair, at the start poses.  The two routes alternate; 2 warm-ups, then the median
of 5.  Both routes need one full evaluation: it is timed on its own (a solve of zero iterations) and is part of (a)
only, as the call makes it; (b) starts from the system that evaluation left on the device.  The split of (a) is by
difference: a call for the one pair (last free node, last free node) evaluates and factorises like any other but
solves four columns over one panel, so factorisation = that call - evaluation and solves = all pairs - that call.
Launches are counted from the shapes (3 per panel less 2 for the factorisation, 4 for unit columns, two substitutions
and the gather).  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script of its own
(--only library).  Usage: python profiles/pose_graph_covariance_bench.py [--out profiles/pose_graph_covariance.txt]"""
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


def host_route(pg, n, pairs):
    """download H, invert it on the host, cut the blocks out (node 0 alone is constant: free position = node - 1)"""
    t0 = time.perf_counter()
    H, _ = pg.download_system()
    t1 = time.perf_counter()
    inv = np.linalg.inv(H)
    t2 = time.perf_counter()
    out = np.zeros((len(pairs), 4, 4))
    for p, (a, b) in enumerate(pairs):
        if a > 0 and b > 0:
            out[p] = inv[4 * a - 4:4 * a, 4 * b - 4:4 * b]
    t3 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2)


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("both", "library"), default="both")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import pose_graph_bench
    from voxgraph_amd import capi
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lines = []
    for name, grid, loop_every in (("config-3 shape", (20, 10), 0), ("config-5 shape", (100, 10), 50)):
        n, poses, pairs, batch, edges = pose_graph_bench.build(capi, ctx, grid, loop_every)
        pg = capi.PoseGraph(ctx, n)
        pg.set_registration(batch)
        pg.set_edges([capi.pose_graph_edge(*e) for e in edges])
        nf = 4 * (n - 1)
        rows = []
        for r in range(a.warmup + a.repeats):
            _, t_eval = timed(lambda: pg.optimize(poses, max_num_iterations=0))
            _, t_one = timed(lambda: pg.covariance(poses, [(n - 1, n - 1)]))
            blocks, t_all = timed(lambda: pg.covariance(poses, pairs))
            host = None
            if a.only == "both":
                host, t_host = host_route(pg, n, pairs)
            if r >= a.warmup:
                rows.append((t_eval, t_one, t_all) + (t_host if host is not None else (0.0, 0.0, 0.0)))
        med = [statistics.median(row[k] for row in rows) * 1e3 for k in range(6)]
        n_panels = (nf + 63) // 64
        seconds = len({b for a_, b in pairs if a_ > 0 and b > 0})
        lines.append(f"{name}: {n} nodes, {len(pairs)} pairs, {nf} unknowns, {4 * seconds} columns solved, {n_panels} panels")
        lines.append(f"  (a) vgx_pose_graph_covariance, all pairs: {med[2]:9.2f} ms = evaluation {med[0]:8.2f} + factorisation "
                     f"{med[1] - med[0]:8.2f} + solves and gather {med[2] - med[1]:8.2f}; {3 * n_panels - 2} + 4 launches after the evaluation")
        if a.only == "both":
            worst = np.abs(blocks - host).max() / np.abs(host).max()
            lines.append(f"  (b) download_system + numpy.linalg.inv + extraction: {sum(med[3:]):9.2f} ms = download {med[3]:8.2f} + inverse "
                         f"{med[4]:8.2f} + extraction {med[5]:8.2f} (the evaluation not counted); with it {med[0] + sum(med[3:]):9.2f} ms")
            lines.append(f"  (a) against (b): largest block difference {worst:.2e} of the largest entry")
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
