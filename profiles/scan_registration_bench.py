"""Scan-to-map registration on bench.py's two TSDF scenes (harness/bench_tsdf.py: the 10 x 8 x 4 m room seen by an
OS1-64-shaped LiDAR, 64 x 1024 points at 0.20 m voxels with the shipped yaml, and by a 640 x 480 depth camera at 0.05 m
voxels).  Per scene: the racing integrator builds the layer from the session's first scans (its time per scan, host
clock around the queued scans and one synchronise, is printed for scale); the last scan, resident on the device, is registered from a prior
off by a third of the layer's truncation distance in x and y, a sixth in z, and the yaw that moves a point 4 m away by a
third of it (what such a cost can pull in scales with the truncation distance: beyond it a point sees the plateau).  Host clock around each call -- every evaluate / refine ends in a device
synchronise -- median of --reps after warm-up:

  evaluate    one vgx_scan_registration_evaluate at the prior: two launches, one 136-byte copy, one synchronisation
  refine      a whole vgx_scan_registration_refine: iterations, evaluations, and the time per evaluation

    python profiles/scan_registration_bench.py [--reps 200] [--out profiles/scan_registration.txt]
Kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (--reps 20 is enough there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from harness.bench_tsdf import sensor_cases, session_scans  # noqa: E402
from voxgraph_amd import capi  # noqa: E402


def _ms(fn, reps, warmup=5):
    out, times = None, []
    for _ in range(warmup + reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, times[warmup:]


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--scans", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_registration.txt"))
    args = ap.parse_args()
    ctx = capi.Context(0)
    lines = []
    for name, (dirs, vs, kw, _, _) in sensor_cases().items():
        poses, clouds = session_scans(dirs, args.scans)
        n = clouds[0].shape[0]
        reach = kw["max_ray_length_m"] + kw["default_truncation_distance"] + 2 * vs
        layer = capi.TsdfLayer(ctx, vs, 16)
        for k in (0, args.scans - 1):
            layer.reserve(poses[k][4:7], reach)
        integrator = capi.FastTsdfIntegrator(ctx, capi.tsdf_config(**kw), layer)
        dev = [torch.from_numpy(c).cuda() for c in clouds]
        torch.cuda.synchronize()
        integrator.integrate_device(poses[0], dev[0].data_ptr(), None, n)      # warm-up scan
        ctx.synchronize_tsdf()
        t = time.perf_counter()
        for k in range(1, args.scans - 1):
            integrator.integrate_device(poses[k], dev[k].data_ptr(), None, n)
        ctx.synchronize_tsdf()
        integrate_ms = (time.perf_counter() - t) * 1e3 / (args.scans - 2)
        # the last scan, from a drifted prior
        true = poses[-1].astype(np.float64)
        off = kw["default_truncation_distance"] / 3.0
        yaw_true = 2.0 * np.arctan2(true[3], true[0])
        yaw = yaw_true + off / 4.0
        prior = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), true[4] + off, true[5] - off, true[6] + off / 2], np.float32)
        reg = capi.ScanRegistration(ctx, capi.scan_registration_config(0.9 * kw["default_truncation_distance"]))
        reg.set_points(dev[-1])
        (out, n_valid, n_cand), t_eval = _ms(lambda: reg.evaluate(layer, prior), args.reps)
        (T, usable, delta, S), t_refine = _ms(lambda: reg.refine(layer, prior), max(10, args.reps // 4))
        err0 = float(np.linalg.norm(prior[4:7].astype(np.float64) - true[4:7]))
        err1 = float(np.linalg.norm(T[4:7].astype(np.float64) - true[4:7]))
        yaw1 = 2.0 * np.arctan2(float(T[3]), float(T[0]))
        row = {"scene": name, "points": n, "voxel_size": vs, "candidates": n_cand, "usable_at_prior": n_valid,
               "workgroups": -(-n // 1024), "evaluate": _stat(t_eval), "refine": _stat(t_refine),
               "refine_iterations": S["num_iterations"], "refine_evaluations": S["num_evaluations"], "refine_usable": bool(usable),
               "refine_ms_per_evaluation": round(float(np.median(t_refine)) / S["num_evaluations"], 4),
               "refine_evaluation_seconds_share": round(S["evaluation_seconds"] / max(S["total_seconds"], 1e-12), 3),
               "prior_error_m": round(err0, 4), "refined_error_m": round(err1, 4),
               "refined_yaw_error_rad": round(abs(yaw1 - yaw_true), 5), "prior_yaw_error_rad": round(off / 4.0, 5),
               "racing_integrator_ms_per_scan_host_clock": round(integrate_ms, 4), "reps": args.reps}
        lines.append(json.dumps(row))
        print(lines[-1])
        for h in (reg, integrator, layer):
            h.destroy()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# python profiles/scan_registration_bench.py --reps %d  (one JSON line per scene; host clock, every call ends in a "
                "device synchronise)\n" % args.reps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
