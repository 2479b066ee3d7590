"""LiDAR range-image integration against the two routes a LiDAR scan could take before it, per scan, from a decoded scan
that is resident on the device:

  range_image     vgx_range_image_build (queued) + vgx_tsdf_integrate_range_image, counted (the call ends in the read-back)
  racing          vgx_tsdf_integrate_scan, racing mode, counted
  reproducible    the same with vgx_tsdf_config.deterministic = 1

Scenes: a sensor 1.8 m above a street between two facades 16 m apart (the street's ends lie beyond the rays' 16 m), swept at
64 x 1024 and 128 x 2048 with the settings of voxgraph_mapper.yaml (0.20 m voxels, rays up to 16 m, truncation 0.6 m); a
room of 10 x 8 x 3 m at the same settings and at 0.10 m voxels with truncation 0.3 m; 16 voxels a side.  One return per
pixel, a quarter pitch of jitter.  Every route has its own layer and integrates the same scan from the same pose again and
again: the steady state of a sensor that looks at a mapped place (no block is new after the first scan).  Host clock around
calls that end in a synchronisation; WARMUP rounds, then --reps timed rounds with the routes alternating in one process so
that all see the same machine; median with the 10th / 90th percentile.  The clocks are whatever the device runs at under
this load: the script prints what rocm-smi reports before and after (it sets nothing).
The kernels' own times and the launch count come from a kernel trace of --only range_image, taken in a run of its own.

    python profiles/range_image_time.py [--reps 100] [--only range_image]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import range_image_ref as R  # noqa: E402
from tests import range_image_scenes as S  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

WARMUP = 10
VPS = 16
STREET = (np.array([-40.0, -8.0, -1.8]), np.array([40.0, 8.0, 60.0]))
ROOM = (np.array([-4.0, -3.0, -1.2]), np.array([6.0, 5.0, 1.8]))
YAML = dict(default_truncation_distance=0.6, max_ray_length_m=16.0, use_const_weight=1, use_weight_dropoff=1)
# name -> (box, width, height, voxel size, config)
SCENES = {
    "street 64x1024": (STREET, 1024, 64, 0.20, YAML),
    "street 128x2048": (STREET, 2048, 128, 0.20, YAML),
    "room 64x1024 yaml": (ROOM, 1024, 64, 0.20, YAML),
    "room 64x1024 0.10 m": (ROOM, 1024, 64, 0.10, dict(YAML, default_truncation_distance=0.3)),
}
POSE = S.pose(S.quat([0, 0, 1], 0.3), [0.4, -0.3, 0.1])


def sweep(model, box, seed):
    """one return per pixel from the inside of an axis-aligned box around the sensor, in the sensor frame"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(model.height), np.arange(model.width), indexing="ij")
    d = model.centre(u + rng.uniform(-0.25, 0.25, u.shape), v + rng.uniform(-0.25, 0.25, v.shape)).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, box[1] / d, np.where(d < 0, box[0] / d, np.inf)).min(1)
    pts = (d * t[:, None]).astype(np.float32)
    return pts, rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)


def _clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return " | ".join(line.strip() for line in out.splitlines() if "sclk" in line or "mclk" in line)[:400]
    except Exception as e:  # (a report, not a measurement: never fatal)
        return f"not available ({type(e).__name__})"


def _stat(times):
    q = np.percentile(times, [10, 50, 90])
    return {"median_ms": round(float(q[1]), 4), "p10_ms": round(float(q[0]), 4), "p90_ms": round(float(q[2]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--only", default="")
    ap.add_argument("--scene", default="")
    args = ap.parse_args()
    print("clocks before:", _clocks(), flush=True)
    ctx = capi.Context(0)
    lib, C = ctx.lib, capi.C
    Tp = POSE.ctypes.data_as(capi.f32p)
    rows = []
    for name, (box, width, height, vs, settings) in SCENES.items():
        if args.scene and args.scene not in name:
            continue
        model = R.Model(width, height, float(R.PI), 1, 0.3927, -0.3927)
        lidar = model.capi(capi)
        pts, rgba = sweep(model, box, width)
        data, layout = S.message(pts, rgba)
        scan = capi.Scan(ctx)
        scan.decode_msg(capi.scan_layout(**layout), data)
        handles, routes, info = [scan], {}, {}

        def rig(**kw):
            layer = capi.TsdfLayer(ctx, vs, VPS)
            integ = capi.FastTsdfIntegrator(ctx, capi.tsdf_config(**settings, **kw), layer)
            handles.extend([integ, layer])
            return layer, integ

        layer, integ = rig()
        image = capi.RangeImage(ctx)
        handles.insert(0, image)
        counts = capi.ProjectiveCounts()

        def range_image(integ=integ, counts=counts):
            rc = lib.vgx_range_image_build(image.h, C.byref(lidar), scan.h, None)
            return rc or lib.vgx_tsdf_integrate_range_image(integ.h, Tp, image.h, C.byref(counts))
        routes["range_image"] = range_image
        info["range_image"] = layer
        for mode, det in (("racing", 0), ("reproducible", 1)):
            layer, integ = rig(deterministic=det)
            n = C.c_int64()

            def raycast(integ=integ, n=n):
                return lib.vgx_tsdf_integrate_scan(integ.h, Tp, scan.h, 0, C.byref(n))
            routes[mode] = raycast
            info[mode] = layer
        routes = {k: v for k, v in routes.items() if k.startswith(args.only)}
        t = {k: [] for k in routes}
        first = {}
        for k in range(WARMUP + args.reps):
            for key, fn in routes.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = time.perf_counter() - t0
                assert rc == 0, (key, rc)
                if k == 0:
                    first[key] = round(dt * 1e3, 3)
                if k >= WARMUP:
                    t[key].append(dt * 1e3)
        res = {"scene": name, "points": len(pts), "reps": args.reps, "voxel_size": vs, "vps": VPS, "first_call_ms": first}
        res["projective_counts"] = {k: getattr(counts, k) for k, _ in capi.ProjectiveCounts._fields_}
        ic = image.stats()
        res["image_counts"] = {k: int(ic[k]) for k in ("n_points", "n_kept", "n_filled", "n_collided")}
        res["blocks"] = {k: info[k].stats()[0] for k in routes}
        res.update({key: _stat(v) for key, v in t.items()})
        print(json.dumps(res), flush=True)
        rows.append((res, list(routes)))
        for h in handles:
            h.destroy()
    print("clocks after:", _clocks())
    print()
    print("median ms (p10 .. p90) per scan")
    for res, keys in rows:
        print(res["scene"], "  ".join("%s %.3f (%.3f .. %.3f)" % (k, res[k]["median_ms"], res[k]["p10_ms"], res[k]["p90_ms"]) for k in keys))
    ctx.close()


if __name__ == "__main__":
    main()
