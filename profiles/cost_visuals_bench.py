"""Cost of the cost-function visuals on one 256^3 kVoxels pair of the bench's scene generator (bench.py's defaults):
  visuals   vgx_reg_evaluate_visuals: the rows and, in one more kernel, the residual cloud and the Jacobian markers, then
            their download (vgx_reg_visuals_download)
  parent    the route before it existed: vgx_reg_evaluate, then a plain single-thread C++ loop
            (profiles/cost_visuals_host_loop.cpp) that builds the same three arrays from the f64 rows
The two routes run alternating; the medians and the run count are printed.  `--kernel-only K` evaluates K times and
exits (for a `rocprofv3 --kernel-trace --stats` run of its own: the kernel time in profiles/cost_visuals.txt).
Measured: profiles/cost_visuals.txt."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))


def host_loop():
    so = os.path.join(tempfile.mkdtemp(prefix="cost_visuals_"), "host_loop.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", os.path.join(HERE, "cost_visuals_host_loop.cpp"),
                           "-o", so])
    fn = C.CDLL(so).cost_visuals_host_loop
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    fn.argtypes = [C.c_int64, f32p, f64p, f64p, C.c_double, f32p, f32p, C.c_void_p, f64p, f64p]
    fn.restype = None
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    from oracle import pyoracle as orc
    from voxgraph_amd import capi
    ctx = capi.Context(0)
    true_poses = [np.array([0.0, 0.0, 0.0, 0.0]), np.array([1.1, -0.7, 0.1, 0.03])]
    subs = []
    for k in range(2):
        sm = capi.Submap.synth_city(ctx, k, 0.2, 16, [-8, -8, -4], [16, 16, 16], 0.6, 2.0, 10.0, true_poses[k], 2)
        sm.extract_voxel_points(1.0, 0.3, True)
        subs.append(sm)
    ctx.synchronize()
    cf = capi.RegistrationCostFunction(ctx, subs[0], subs[1], capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    vis = capi.RegVisuals(ctx)
    n = cf.num_residuals()
    ref_pose, read_pose = true_poses[0] + np.array([0.05, -0.04, 0.02, 0.01]), true_poses[1]
    r, jo, je = np.zeros(n), np.zeros((n, 4)), np.zeros((n, 4))
    if args.kernel_only:
        for _ in range(args.kernel_only):
            assert cf.evaluate_visuals([ref_pose, read_pose], r, [jo, je], vis)
        print(json.dumps({"rows": n, "evaluations": args.kernel_only}))
        return
    xyz, _, w = subs[0].download_points(capi.POINTS_VOXELS)
    xyz = np.ascontiguousarray(xyz, np.float32)
    factor = float(n / np.sum(w.astype(np.float64)))
    q, t = orc.relative_transform(ref_pose, read_pose)
    rel = np.array([q[0], q[3], *t], np.float32)
    q, t = orc.relative_transform(read_pose, np.zeros(4))
    mission = np.array([q[0], q[3], *t], np.float32)
    loop = host_loop()
    cloud_h, arrows_h, origins_h = np.zeros((n, 32), np.uint8), np.zeros((2 * n, 3)), np.zeros((n, 3))
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)

    def visuals_route():
        t0 = time.perf_counter()
        assert cf.evaluate_visuals([ref_pose, read_pose], r, [jo, je], vis)
        t1 = time.perf_counter()
        out = vis.download()
        return t1 - t0, time.perf_counter() - t1, out

    def parent_route():
        t0 = time.perf_counter()
        assert cf.Evaluate([ref_pose, read_pose], r, [jo, je])
        t1 = time.perf_counter()
        loop(n, xyz.ctypes.data_as(f32p), r.ctypes.data_as(f64p), je.ctypes.data_as(f64p), factor, rel.ctypes.data_as(f32p),
             mission.ctypes.data_as(f32p), cloud_h.ctypes.data, arrows_h.ctypes.data_as(f64p), origins_h.ctypes.data_as(f64p))
        return t1 - t0, time.perf_counter() - t1

    visuals_route(), parent_route()  # warm-up: allocations, first launches
    v, p = [], []
    for _ in range(args.runs):
        v.append(visuals_route())
        p.append(parent_route())
    out = v[-1][2]
    same_positions = bool(np.array_equal(out[0].view(np.float32).reshape(n, 8)[:, :3], cloud_h.view(np.float32).reshape(n, 8)[:, :3]))
    med = lambda xs: statistics.median(xs) * 1e3
    res = {"rows": n, "runs": args.runs, "factor": factor,
           "visuals_evaluate_ms": med([a for a, _, _ in v]), "visuals_download_ms": med([b for _, b, _ in v]),
           "visuals_total_ms": med([a + b for a, b, _ in v]),
           "parent_evaluate_ms": med([a for a, _ in p]), "parent_host_loop_ms": med([b for _, b in p]),
           "parent_total_ms": med([a + b for a, b in p]),
           "bytes_written_per_row": 104, "positions_equal_host_loop": same_positions}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
