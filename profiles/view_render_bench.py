"""View rendering on bench.py's two TSDF scenes (harness/bench_tsdf.py: the 10 x 8 x 4 m room seen by an OS1-64-shaped
LiDAR, 64 x 1024 rays over a 0.20 m layer built with the shipped yaml, and by a 640 x 480 depth camera over a 0.05 m layer).
Per scene the racing integrator builds the layer from the session's scans; the view is rendered from the last scan's pose
along the sensor's own rays (resident on the device), with min_step = voxel_size / 4, unknown_step = voxel_size,
max_bracket = the truncation distance and s_max = the integrator's max_ray_length_m, once with rays mapped to lanes by
index and once by 8 x 8 image tiles.  Host clock around each call -- every render ends in a device synchronise -- median
of --reps after warm-up.  Per row:

  ms per view, rays/s, samples/s, and samples x 64 B / time (a sample gathers 8 voxels of 8 bytes: the traffic the
  march asks for, not what reaches HBM -- neighbouring rays share voxels); mean and max samples per ray; the wave
  efficiency sum(samples) / (64 x sum of per-wave maxima) of that mapping, from n_samples; the shares of the statuses

    python profiles/view_render_bench.py [--reps 100] [--out profiles/view_render.txt]
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

SHAPES = {"rgbd_640x480_0.05m": (640, 480), "lidar_64x1024_0.20m_voxgraph_yaml": (1024, 64)}


def wave_efficiency(n_samples, width):
    """rays to waves by index (width 0), or by 8 x 8 tiles of an image `width` wide (the kernel's two mappings)"""
    s = np.asarray(n_samples, np.int64)
    if width > 0:
        rows = -(-len(s) // width)
        img = np.zeros((-(-rows // 8) * 8, -(-width // 8) * 8), np.int64)
        flat = np.zeros(rows * width, np.int64)
        flat[:len(s)] = s
        img[:rows, :width] = flat.reshape(rows, width)
        waves = img.reshape(img.shape[0] // 8, 8, img.shape[1] // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    else:
        pad = np.zeros(-(-len(s) // 64) * 64, np.int64)
        pad[:len(s)] = s
        waves = pad.reshape(-1, 64)
    return float(s.sum()) / float(64 * waves.max(1).sum())


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--scans", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_render.txt"))
    args = ap.parse_args()
    ctx = capi.Context(0)
    lines = []
    for name, (dirs, vs, kw, _, _) in sensor_cases().items():
        width, height = SHAPES[name]
        poses, clouds = session_scans(dirs, args.scans)
        n = clouds[0].shape[0]
        assert n == width * height
        reach = kw["max_ray_length_m"] + kw["default_truncation_distance"] + 2 * vs
        layer = capi.TsdfLayer(ctx, vs, 16)
        for k in (0, args.scans - 1):
            layer.reserve(poses[k][4:7], reach)
        integrator = capi.FastTsdfIntegrator(ctx, capi.tsdf_config(**kw), layer)
        for k in range(args.scans):
            integrator.integratePointCloud(poses[k], clouds[k])
        d_dirs = torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).cuda()
        torch.cuda.synchronize()
        truth = np.linalg.norm(clouds[-1].astype(np.float64), axis=1)
        cfg = dict(s_max=kw["max_ray_length_m"], min_step=vs / 4, unknown_step=vs, max_bracket=kw["default_truncation_distance"])
        images = []
        for mapping, image_width in (("index", 0), ("tiles_8x8", width)):
            view = capi.View(ctx, capi.view_config(flags=capi.VIEW_POINTS | capi.VIEW_N_SAMPLES, image_width=image_width, **cfg))
            times = []
            for _ in range(5 + args.reps):
                t = time.perf_counter()
                layer.render_view(view, poses[-1], d_dirs)
                times.append((time.perf_counter() - t) * 1e3)
            times = times[5:]
            ms = float(np.median(times))
            c, image = view.stats(), view.download()
            images.append(image)
            hit = (image.status == capi.VIEW_HIT) | (image.status == capi.VIEW_HIT_UNSAMPLED)
            err = np.abs(image.range[hit].astype(np.float64) - truth[hit])
            row = {"scene": name, "mapping": mapping, "rays": n, "voxel_size": vs, "ms_per_view": round(ms, 4),
                   "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
                   "rays_per_s": round(n / (ms * 1e-3)), "samples_per_s": round(c["n_samples"] / (ms * 1e-3)),
                   "gathered_GB_per_s": round(c["n_samples"] * 64 / (ms * 1e-3) / 1e9, 2),
                   "samples_mean": round(c["n_samples"] / n, 3), "samples_max": int(image.n_samples.max()),
                   "wave_efficiency": round(wave_efficiency(image.n_samples, image_width), 4),
                   "hit": round(c["n_hit"] / n, 4), "hit_unsampled": round(c["n_hit_unsampled"] / n, 4), "miss": round(c["n_miss"] / n, 4),
                   "inside": round(c["n_inside"] / n, 4), "median_range_error_m": round(float(np.median(err)), 5) if hit.any() else None,
                   "reps": args.reps}
            lines.append(json.dumps(row))
            print(lines[-1])
            view.destroy()
        for a, b in zip(images[0], images[1]):                         # the mapping never changes a result
            assert a is None and b is None or np.array_equal(a.view(np.uint8), b.view(np.uint8))
        integrator.destroy()
        layer.destroy()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# python profiles/view_render_bench.py --reps %d  (one JSON line per scene and ray mapping; host clock, every "
                "render ends in a device synchronise)\n" % args.reps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
