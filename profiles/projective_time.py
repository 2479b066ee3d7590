"""Projective depth-image integration against the two routes a depth frame could take before it, per frame:

  projective_host / _device   vgx_tsdf_integrate_depth_image / _device, counted (the call ends in the read-back of the counts)
  racing_host / _device       vgx_scan_decode_depth_image[_device] + vgx_tsdf_integrate_scan, racing mode, counted
  reproducible_host / _device the same with vgx_tsdf_config.deterministic = 1

Frames: a camera inside the room of tests/scan_msg_scenes.py (tests/depth_image_ref.room_frame) at 640 x 480 and 1280 x 720,
16UC1 with a registered RGB8 image, 0.05 m voxels, 16 voxels a side, truncation 0.15 m, rays up to 5 m (the grid and the
settings of bench.py's config 4).  Every route has its own layer and integrates the same frame from the same pose again
and again: the steady state of a camera that looks at a mapped room (no block is new after the first frame).  Host clock
around calls that end in a synchronisation; WARMUP rounds, then --reps timed rounds with the routes alternating in one
process so that all see the same machine; median with the 10th / 90th percentile.  The clocks are whatever the device
runs at under this load: the script prints what rocm-smi reports before and after (it sets nothing).
The kernel's own time, its share of the bound of DESIGN.md 30 and the launch count come from a kernel trace of
--only projective, taken in a run of its own.

    python profiles/projective_time.py [--reps 100] [--only projective]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import depth_image_ref as D  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

WARMUP = 10
VS, VPS = 0.05, 16
SETTINGS = dict(default_truncation_distance=0.15, max_ray_length_m=5.0)


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
    args = ap.parse_args()
    import torch
    print("clocks before:", _clocks(), flush=True)
    ctx = capi.Context(0)
    lib, C = ctx.lib, capi.C
    T = D.T_ROOM_OPTICAL
    Tp = T.ctypes.data_as(capi.f32p)
    rows = []
    for width, height in ((640, 480), (1280, 720)):
        img, cam = D.room_frame(width, height, D.DEPTH_16UC1, seed=width, color_kind=D.COLOR_RGB8, row_pad=0, color_pad=0)
        lay, camera = img.layout(capi), cam.capi(capi)
        depth, color = np.ascontiguousarray(img.depth), np.ascontiguousarray(img.color)
        d_depth, d_color = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        torch.cuda.synchronize()
        handles, routes, info = [], {}, {}

        def rig(**kw):
            layer = capi.TsdfLayer(ctx, VS, VPS)
            integ = capi.FastTsdfIntegrator(ctx, capi.tsdf_config(**SETTINGS, **kw), layer)
            handles.extend([integ, layer])
            return layer, integ

        for form in ("host", "device"):
            dp, cp = (depth.ctypes.data, color.ctypes.data) if form == "host" else (d_depth.data_ptr(), d_color.data_ptr())
            layer, integ = rig()
            counts = capi.ProjectiveCounts()
            fn = lib.vgx_tsdf_integrate_depth_image if form == "host" else lib.vgx_tsdf_integrate_depth_image_device

            def projective(fn=fn, integ=integ, dp=dp, cp=cp, counts=counts):
                return fn(integ.h, Tp, C.byref(lay), C.byref(camera), dp, len(depth), cp, len(color), C.byref(counts))
            routes[f"projective_{form}"] = projective
            info[f"projective_{form}"] = (layer, counts)
            for mode, det in (("racing", 0), ("reproducible", 1)):
                if args.only:
                    continue
                layer, integ = rig(deterministic=det)
                scan = capi.Scan(ctx)
                handles.insert(0, scan)
                decode = lib.vgx_scan_decode_depth_image if form == "host" else lib.vgx_scan_decode_depth_image_device
                n = C.c_int64()

                def raycast(decode=decode, scan=scan, integ=integ, dp=dp, cp=cp, n=n):
                    rc = decode(scan.h, C.byref(lay), C.byref(camera), None, dp, len(depth), cp, len(color))
                    return rc or lib.vgx_tsdf_integrate_scan(integ.h, Tp, scan.h, 0, C.byref(n))
                routes[f"{mode}_{form}"] = raycast
                info[f"{mode}_{form}"] = (layer, n)
        routes = {k: v for k, v in routes.items() if k.startswith(args.only)}
        t = {k: [] for k in routes}
        first = {}
        for k in range(WARMUP + args.reps):
            for key, fn in routes.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = time.perf_counter() - t0
                assert rc == 0, (key, rc, ctx.last_error() if hasattr(ctx, "last_error") else "")
                if k == 0:
                    first[key] = round(dt * 1e3, 3)
                if k >= WARMUP:
                    t[key].append(dt * 1e3)
        res = {"frame": f"{width}x{height}", "reps": args.reps, "voxel_size": VS, "vps": VPS, "first_call_ms": first}
        pc = info["projective_device"][1]
        res["projective_counts"] = {k: getattr(pc, k) for k, _ in capi.ProjectiveCounts._fields_}
        res["blocks"] = {k: info[k][0].stats()[0] for k in routes}
        res.update({key: _stat(v) for key, v in t.items()})
        print(json.dumps(res), flush=True)
        rows.append((res, list(routes)))
        for h in handles:
            h.destroy()
    print("clocks after:", _clocks())
    print()
    print("median ms (p10 .. p90) per frame")
    for res, keys in rows:
        print(res["frame"], "  ".join("%s %.3f (%.3f .. %.3f)" % (k, res[k]["median_ms"], res[k]["p10_ms"], res[k]["p90_ms"]) for k in keys))
    ctx.close()


if __name__ == "__main__":
    main()
