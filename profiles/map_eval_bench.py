"""Map evaluation (MapEvaluation::evaluate: capi.map_evaluation) on the 200-submap scene of
profiles/projected_map_bench.py.  The ground truth is the projected map at the true poses; the evaluated map uses
perturbed poses.  Prints one JSON line: host-clock ms of the transform (vgx_tsdf_layer_transform_submap), the ESDF
regeneration of the transformed ground truth, the evaluation (vgx_evaluate_layers_rmse, with and without the error
layer), the whole evaluate() with the solver's iterations, and the evaluation's byte count against 8 TB/s.

    python profiles/map_eval_bench.py [--reps 5]
Kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxgraph_amd import capi  # noqa: E402


def _ms(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--skip-evaluate", action="store_true", help="time the three device steps only")
    args = ap.parse_args()
    from harness import lm
    from harness.backends import GpuBackend
    gw, gh = args.grid
    vs, vps = args.voxel_size, 16
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
    gt_layer = capi.TsdfLayer(ctx, vs, vps)
    capi.projected_map(ctx, subs, T_true, gt_layer)
    gt = capi.Submap.from_tsdf_layer(ctx, gt_layer, 1000)
    gt_layer.destroy()
    test_layer = capi.TsdfLayer(ctx, vs, vps)
    capi.projected_map(ctx, subs, T_test, test_layer)
    test = capi.Submap.from_tsdf_layer(ctx, test_layer, 1)
    test_layer.destroy()
    test.generate_esdf()
    ctx.synchronize()

    # the device steps of evaluate() after the alignment, one by one, at a small pose
    T = capi.decoupled_exp_pose([0.013, -0.008, 0.004, 0.0015])
    layers = []

    def transform():
        layer = capi.TsdfLayer(ctx, vs, vps)
        layer.transform_submap(gt, T)          # returns once the copy kernel has finished
        layers.append(layer)

    _, t_transform = _ms(transform, args.reps + 1)
    gt_t = capi.Submap.from_tsdf_layer(ctx, layers[-1], 1000)
    for layer in layers:
        layer.destroy()
    _, t_esdf = _ms(lambda: gt_t.generate_esdf(), args.reps + 1)
    det, t_eval = _ms(lambda: capi.evaluate_layers_rmse(gt_t, test, capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_TEST),
                      args.reps + 1)
    _, t_eval_err = _ms(lambda: capi.evaluate_layers_rmse(gt_t, test, capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_TEST,
                                                          True), args.reps + 1)
    n_test, n_gt = test.num_blocks(), gt_t.num_blocks()
    vox = vps ** 3
    eval_bytes = (n_test + n_gt) * vox * 5                  # f32 distance + u8 observed, read once from each layer
    eval_err_bytes = eval_bytes + n_test * vox * 5          # + f32 error distance + u8 set written per error voxel
    out = {"workload": f"map evaluation, {len(subs)} city submaps @ "
                       f"{args.block_dims[0] * 16}x{args.block_dims[1] * 16}x{args.block_dims[2] * 16}",
           "test_blocks": n_test, "gt_blocks": n_gt,
           "transform_ms": [round(x, 2) for x in t_transform[1:]],
           "esdf_regeneration_ms": [round(x, 2) for x in t_esdf[1:]],
           "evaluation_ms": [round(x, 3) for x in t_eval[1:]],
           "evaluation_with_error_layer_ms": [round(x, 2) for x in t_eval_err[1:]],
           "evaluation_bytes": eval_bytes, "evaluation_with_error_layer_bytes": eval_err_bytes,
           "evaluation_floor_ms_at_8_tb_s": round(eval_bytes / 8e12 * 1e3, 3),
           "evaluation_with_error_layer_floor_ms_at_8_tb_s": round(eval_err_bytes / 8e12 * 1e3, 3),
           "details_after_small_transform": det}
    gt_t.destroy()

    if not args.skip_evaluate:
        summary = {}

        def align(reference, reading):
            cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=-1.0, use_esdf_distance=1)
            cf = capi.RegistrationCostFunction(ctx, reference, reading, cfg)
            batch = capi.RegistrationBatch(ctx, [cf], [(0, 1)])
            x, s = lm.solve(lm.Problem(GpuBackend(capi, ctx, batch, 2), 2, [(0, 1)]), np.zeros((2, 4)),
                            parameter_tolerance=1e-12, max_iterations=200, max_seconds=120)
            summary.update(iterations=s["iterations"], termination=s["termination"], solver_s=round(s["seconds"], 3))
            batch.destroy()
            cf.destroy()
            return x[1]

        # the first call also pays for torch's device set-up (the harness backend's buffers) and first-use code loads
        evaluate_ms = []
        for _ in range(3):
            t = time.perf_counter()
            res = capi.map_evaluation(ctx, subs, T_test, gt, align)
            evaluate_ms.append(round((time.perf_counter() - t) * 1e3, 1))
        out["evaluate_ms"] = evaluate_ms
        out["evaluate_solver"] = summary
        out["evaluate_details"] = res["details"]
        out["evaluate_T_ground_truth__reading"] = [round(float(v), 6) for v in res["T_ground_truth__reading"]]
    print(json.dumps(out))
    for h in subs + [gt, test]:
        h.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
