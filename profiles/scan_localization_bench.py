"""Scan localisation on the asymmetric room of tests/scan_localization_scenes.py (0.20 m voxels, 30 blocks, the ESDF
generated on the device) seen by a 64 x 1024 beam scanner at the scene's true pose.  Host clock around each call -- every
one ends in a device synchronise -- median of --reps after warm-up (--reps / 10 for the loops):

  evaluate_map   one vgx_scan_registration_evaluate_map at K = 1, 4, 16 listed submaps (K uploads of the room under the
                 identity pose: every point is usable in every one of them, the most work a point can be)
  score          vgx_scan_registration_score_poses at 1, 64, 1024, 4608 hypotheses against the SAME poses looped through
                 vgx_scan_registration_evaluate_map, both at stride 4 (16384 candidates); the costs are compared bit for bit
  localize       one whole vgx_scan_registration_localize on the 4608-hypothesis grid: scoring at stride 4, the
                 refinement on every point

Each step runs as a process of its own under its own time limit, and the steps are chained: one that fails ends the run.
Nothing is asserted on times but this: from 64 poses up the batched call must be faster than the loop it replaces.

    python profiles/scan_localization_bench.py [--reps 200] [--out profiles/scan_localization.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("evaluate_map", 120), ("score", 240), ("localize", 120))       # (step, its time limit in seconds)


def _ms(fn, reps, warmup=3):
    out, times = None, []
    for _ in range(warmup + reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, times[warmup:]


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def _scene(ctx, copies):
    """(submaps [copies], the 64 x 1024 scan on the device, the hypothesis grid)"""
    import torch
    from tests import scan_localization_ref as R
    from tests import scan_localization_scenes as S
    from voxgraph_amd import capi
    d = S.room_submap()
    submaps = []
    for k in range(copies):
        sm = capi.Submap(ctx, k, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight)
        sm.generate_esdf()
        submaps.append(sm)
    scan = torch.from_numpy(S.room_scan(S.TRUE_POSE, 1024, 64)).cuda()
    torch.cuda.synchronize()
    return submaps, scan, R.hypothesis_grid(S.GRID_X, S.GRID_Y, S.GRID_YAWS, S.GRID_Z), S


def _handle(ctx, submaps, scan, S, **cfg):
    from voxgraph_amd import capi
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(S.MAX_ABS_DISTANCE, **cfg))
    reg.set_map(submaps, np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), (len(submaps), 1)),
                capi.scan_map_config(score_point_stride=4))
    reg.set_points(scan)
    return reg


def step(name, reps):
    from tests import scan_registration_ref as SR
    from voxgraph_amd import capi
    ctx = capi.Context(0)
    rows = []
    if name == "evaluate_map":
        submaps, scan, _, S = _scene(ctx, 16)
        T = SR.pose7(S.TRUE_POSE)
        for K in (1, 4, 16):
            reg = _handle(ctx, submaps[:K], scan, S)
            (out, n_terms, n_valid, n_cand), t = _ms(lambda: reg.evaluate_map(T), reps)
            rows.append({"step": name, "submaps": K, "points": int(scan.shape[0]), "candidates": n_cand, "points_valid": n_valid,
                         "terms": n_terms, "evaluate_map": _stat(t), "reps": reps})
            reg.destroy()
    elif name == "score":
        submaps, scan, grid, S = _scene(ctx, 1)
        batched = _handle(ctx, submaps, scan, S)
        looped = _handle(ctx, submaps, scan, S, point_stride=4)
        for n_poses in (1, 64, 1024, 4608):
            poses = grid[:: len(grid) // n_poses][:n_poses]
            (cost, nt, nv, nc), t_batch = _ms(lambda: batched.score_poses(poses), reps)
            outs, t_loop = _ms(lambda: [looped.evaluate_map(T) for T in poses], max(2, reps // 10), warmup=1)
            same = all(np.float64(0.5 * o[0][0]).tobytes() == np.float64(c).tobytes() for o, c in zip(outs, cost))
            rows.append({"step": name, "poses": n_poses, "candidates_per_pose": int(nc[0]), "score_poses": _stat(t_batch),
                         "evaluate_map_loop": _stat(t_loop), "loop_over_batched": round(float(np.median(t_loop) / np.median(t_batch)), 2),
                         "same_bits": bool(same), "reps": reps, "loop_reps": max(2, reps // 10)})
            if not same or (n_poses >= 64 and not np.median(t_batch) < np.median(t_loop)):
                print(json.dumps(rows[-1]))
                raise SystemExit("the batched call is not faster than the loop it replaces, or their bits differ")
    elif name == "localize":
        submaps, scan, grid, S = _scene(ctx, 1)
        reg = _handle(ctx, submaps, scan, S)
        (best, T, usable, delta, summary), t = _ms(lambda: reg.localize(grid), max(2, reps // 10), warmup=1)
        err = SR.pose_error(T, S.TRUE_POSE)
        rows.append({"step": name, "poses": len(grid), "best_index": best, "usable": bool(usable), "localize": _stat(t),
                     "refine_evaluations": summary["num_evaluations"], "error_m": round(err[0], 4), "error_rad": round(err[1], 6),
                     "reps": max(2, reps // 10)})
    for r in rows:
        print(json.dumps(r))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_localization.txt"))
    ap.add_argument("--step", default=None, help="run one step in this process (the driver's children)")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return
    lines = []
    for name, limit in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)], capture_output=True,
                           text=True, timeout=limit)
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        print(r.stdout, end="")
        if r.returncode != 0:
            print(r.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"step {name} ended with {r.returncode}: nothing more is started")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# python profiles/scan_localization_bench.py --reps %d  (one JSON line per measurement; host clock, every call ends in "
                "a device synchronise)\n" % args.reps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
