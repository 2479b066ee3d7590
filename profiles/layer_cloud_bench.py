"""Layer point clouds on the 200-submap scene of profiles/map_eval_bench.py (ground truth = the projected map at the true
poses, evaluated map = perturbed poses).  Prints one JSON line, host clock around each call (every call ends in a device
synchronise), median of --reps after warm-up:

  error slice   vgx_evaluate_layers_rmse_cloud (slice axis 2 at 3 * voxel_size) + download, against the route without it:
                vgx_evaluate_layers_rmse with the error layer copied to the host, then a numpy filter (blocks the plane
                touches first, then their voxels)
  full error cloud, ground truth's surface cloud (TSDF, 0.6 m): the producing call and the download apart, point counts
  byte floors at 8 TB/s: what count and emit read of the layer (all of it, or for a slice the rows the plane touches)
                plus the 16 B per point written

    python profiles/layer_cloud_bench.py [--reps 20]
Kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (--reps 3 is enough there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxgraph_amd import capi  # noqa: E402

F = np.float32


def _ms(fn, reps, warmup=2):
    out, times = None, []
    for _ in range(warmup + reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, times[warmup:]


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}


def host_slice(vs, vps, bi, d, st, axis, plane):
    """the slice of an error layer on the host: blocks whose rows touch the plane, then their observed voxels"""
    vs = F(vs)
    reach = F(0.5) * vs + F(1e-6)
    rows = (np.arange(vps, dtype=F) + F(0.5)) * vs
    c = bi[:, axis].astype(F)[:, None] * (F(vps) * vs) + rows[None]           # [n][vps]
    hit = np.abs(c - F(plane)) <= reach
    blocks = np.flatnonzero(hit.any(1))
    lin = np.arange(vps ** 3)
    idx = (lin // (vps ** axis)) % vps
    keep = hit[blocks][:, idx] & (st[blocks] != 0)
    b, v = np.nonzero(keep)
    ijk = np.stack([v % vps, (v // vps) % vps, v // (vps * vps)], -1).astype(F)
    xyz = bi[blocks][b].astype(F) * (F(vps) * vs) + (ijk + F(0.5)) * vs
    return xyz, d[blocks][b, v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
    gw, gh = args.grid
    vs, vps = args.voxel_size, 16
    vox = vps ** 3
    rng = np.random.default_rng(args.seed)
    extent = np.array(args.block_dims) * 16 * vs
    poses = [[i * extent[0] * 0.5, j * extent[1] / 3.0, 0.0, rng.uniform(-0.1, 0.1)] for j in range(gh) for i in range(gw)]
    ctx = capi.Context(0)
    subs = [capi.Submap.synth_city(ctx, k, vs, vps, args.block_min, args.block_dims, 0.6, 2.0, 10.0, np.array(p), args.seed)
            for k, p in enumerate(poses)]

    def pose7(p):
        return [np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]]

    T_true = np.array([pose7(p) for p in poses], np.float32)
    noisy = [np.array(p) + np.r_[rng.normal(0, 0.02, 3), rng.normal(0, 0.002)] for p in poses]
    T_test = np.array([pose7(p) for p in noisy], np.float32)
    maps = []
    for k, T in ((1000, T_true), (1, T_test)):
        layer = capi.TsdfLayer(ctx, vs, vps)
        capi.projected_map(ctx, subs, T, layer)
        sm = capi.Submap.from_tsdf_layer(ctx, layer, k)
        layer.destroy()
        sm.generate_esdf()
        maps.append(sm)
    gt, test = maps
    for h in subs:
        h.destroy()
    ctx.synchronize()
    n_test, n_gt = test.num_blocks(), gt.num_blocks()
    E, M = capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_TEST
    cloud = capi.Cloud(ctx)
    plane = 3 * vs
    slice_cfg = capi.cloud_config(slice_axis=2, slice_value=plane)

    # ---- the error slice, end to end --------------------------------------------------------------------------------------
    def new_slice():
        det, _ = capi.evaluate_layers_rmse_cloud(gt, test, E, M, slice_cfg, cloud)
        return det, cloud.download()

    def old_slice():
        det, (bi, d, st) = capi.evaluate_layers_rmse(gt, test, E, M, error_layer=True)
        return det, host_slice(vs, vps, bi, d, st, 2, plane), len(bi)

    # alternating, so that both see the same machine
    t_new, t_old = [], []
    for k in range(2 + args.reps):
        (a, ta), (b, tb) = _ms(new_slice, 1, 0), _ms(old_slice, 1, 0)
        if k >= 2:
            t_new += ta
            t_old += tb
    (det_new, (xyz_new, inten_new, _)), (det_old, (xyz_old, inten_old), n_err) = a, b
    same = bool(det_new == det_old and np.array_equal(xyz_new.view(np.uint8), np.ascontiguousarray(xyz_old, F).view(np.uint8)) and
                np.array_equal(inten_new.view(np.uint8), np.ascontiguousarray(inten_old, F).view(np.uint8)))
    _, t_old_copy = _ms(lambda: capi.evaluate_layers_rmse(gt, test, E, M, error_layer=True), max(3, args.reps // 4), 1)
    eval_bytes = (n_test + n_gt) * vox * 5 + n_err * vox * 5       # both layers read, the error layer written (device scratch)
    rows_hit = 1                                                    # rows of a touched block within reach of the plane (of 16)
    touched = int(np.unique(xyz_new[:, 2]).size)
    slice_blocks = int(np.unique(np.floor(xyz_new / F(vps * vs)).astype(np.int64), axis=0).shape[0])
    slice_read = slice_blocks * (vox // vps) * max(touched, rows_hit) * 5
    out = {"workload": f"layer point clouds, {len(poses)} city submaps @ "
                       f"{args.block_dims[0] * 16}x{args.block_dims[1] * 16}x{args.block_dims[2] * 16}",
           "test_blocks": n_test, "gt_blocks": n_gt, "error_blocks": n_err, "reps": args.reps,
           "error_slice": {"points": int(len(xyz_new)), "blocks_contributing": slice_blocks, "rows_in_reach": touched,
                           "new_route": _stat(t_new), "route_without": _stat(t_old),
                           "route_without_evaluation_and_copy_only": _stat(t_old_copy),
                           "ratio_without_over_new": round(float(np.median(t_old) / np.median(t_new)), 1),
                           "results_identical": same,
                           "evaluation_bytes": eval_bytes,
                           "cloud_bytes_count_plus_emit_plus_points": 2 * slice_read + 16 * int(len(xyz_new))}}
    out["error_slice"]["floor_ms_at_8_tb_s"] = round((eval_bytes + out["error_slice"]["cloud_bytes_count_plus_emit_plus_points"]) / 8e12 * 1e3, 4)

    # ---- the full error cloud and the ground truth's surface cloud: the producing call and the download apart --------------
    def timed_cloud(name, produce, layer_bytes, extra_bytes=0):
        _, t_call = _ms(produce, args.reps)
        n = cloud.stats()[0]
        _, t_down = _ms(lambda: cloud.download(), max(3, args.reps // 4), 1)
        cloud_bytes = 2 * layer_bytes + 16 * n                     # count and emit each read the layer; 16 B per point written
        out[name] = {"points": n, "point_bytes": 16 * n, "call": _stat(t_call), "download": _stat(t_down),
                     "cloud_bytes_count_plus_emit_plus_points": cloud_bytes,
                     "floor_ms_at_8_tb_s": round((cloud_bytes + extra_bytes) / 8e12 * 1e3, 4)}

    timed_cloud("full_error_cloud", lambda: capi.evaluate_layers_rmse_cloud(gt, test, E, M, capi.cloud_config(), cloud),
                n_err * vox * 5, eval_bytes)
    timed_cloud("gt_surface_cloud",
                lambda: gt.layer_cloud("tsdf", capi.cloud_config(kind=capi.CLOUD_SURFACE_DISTANCE, surface_distance=0.6), cloud),
                n_gt * vox * 8)
    timed_cloud("gt_esdf_slice", lambda: gt.layer_cloud("esdf", slice_cfg, cloud), 0)
    _, t_eval = _ms(lambda: capi.evaluate_layers_rmse(gt, test, E, M), args.reps)
    out["evaluation_without_error_layer"] = _stat(t_eval)
    print(json.dumps(out))
    for h in (cloud, gt, test):
        h.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
