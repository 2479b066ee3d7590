"""The per-frame path from "message in host memory" to the integrated layer, with and without vgx_scan.  Prints one JSON
line; host clock, median of --reps after warm-up, the two routes alternating so that both see the same machine:

  route without  a plain single-thread C++ pass over the message (profiles/scan_msg_host_convert.cpp, g++ -O2: filter +
                 colour + pack), then vgx_tsdf_integrate of its arrays -- what a caller has to do without vgx_scan
  new route      vgx_scan_decode_msg of the raw bytes, then vgx_tsdf_integrate_scan
  per route      "queued": until the integrate call returns (the scan is queued, n_updates == NULL); "ready": until
                 vgx_ctx_synchronize_tsdf has returned as well
  also           the host pass alone; the decode alone from host bytes and from device bytes (the latter is the kernel,
                 its launch and the call's one synchronisation with the 16-byte read-back: the kernel's own time comes
                 from a rocprofv3 --kernel-trace --stats run of `--profile-only`); bytes the decode moves on the device
                 against (point_step + 16 * kept / n) B per point; both routes' layers compared
Inputs: the 64 x 1024 XYZI LiDAR cloud and the 640 x 480 XYZRGB depth cloud of tests/scan_msg_scenes.py.

    python profiles/scan_msg_bench.py [--reps 50]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/scan_msg_bench.py --profile-only"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scan_msg_ref as R  # noqa: E402
from tests import scan_msg_scenes as S  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

F = np.float32


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def _host_pass(tmp):
    lib = os.path.join(tmp, "libscan_msg_host_convert.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", os.path.join(ROOT, "profiles", "scan_msg_host_convert.cpp"),
                           "-o", lib])
    fn = C.CDLL(lib).host_convert
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p] + [C.c_uint32] * 7 + [C.c_int32, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--profile-only", action="store_true", help="20 decodes per input and nothing else (for rocprofv3)")
    args = ap.parse_args()
    ctx = capi.Context(0)
    scan = capi.Scan(ctx)
    inputs = {"lidar_64x1024_xyzi": S.lidar(0), "depth_640x480_xyzrgb": S.depth(0)}
    if args.profile_only:
        for m in inputs.values():
            for _ in range(20):
                scan.decode_msg(m.layout(capi), m.data)
        scan.destroy()
        ctx.close()
        return
    import torch
    tmp = tempfile.mkdtemp()
    convert = _host_pass(tmp)
    cfg = capi.voxgraph_tsdf_config()
    T = np.array([1, 0, 0, 0, 0.1, -0.05, 0.02], F)
    out = {"reps": args.reps}
    for name, m in inputs.items():
        lay = m.layout(capi)
        data = np.ascontiguousarray(m.data)
        pts, rgba = np.zeros((m.n, 3), F), np.zeros((m.n, 4), np.uint8)

        def host_pass():
            return convert(data.ctypes.data, m.width, m.height, m.point_step, m.row_step, m.offset_x, m.offset_y, m.offset_z,
                           m.color_kind, m.color_offset, 0.0, 10000.0, pts.ctypes.data, rgba.ctypes.data)

        want = R.decode(m)
        n = host_pass()
        assert n == len(want[0]) and np.array_equal(pts[:n].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(rgba[:n], want[1])
        layers = [capi.TsdfLayer(ctx, 0.2, 16) for _ in range(2)]
        integ = [capi.FastTsdfIntegrator(ctx, cfg, l) for l in layers]

        def without():
            t0 = time.perf_counter()
            k = host_pass()
            integ[0].integratePointCloud(T, pts[:k], rgba[:k], count=False)
            t1 = time.perf_counter()
            ctx.synchronize_tsdf()
            return t1 - t0, time.perf_counter() - t0

        def new():
            t0 = time.perf_counter()
            scan.decode_msg(lay, data)
            integ[1].integrate_scan(T, scan, count=False)
            t1 = time.perf_counter()
            ctx.synchronize_tsdf()
            return t1 - t0, time.perf_counter() - t0

        t = {"without": ([], []), "new": ([], [])}
        for k in range(5 + args.reps):
            for key, fn in (("without", without), ("new", new)):
                q, r = fn()
                if k >= 5:
                    t[key][0].append(q * 1e3)
                    t[key][1].append(r * 1e3)

        def timed(fn, reps=args.reps, warmup=3):
            ts = []
            for k in range(warmup + reps):
                t0 = time.perf_counter()
                fn()
                if k >= warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return _stat(ts)

        d = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        kept = len(want[0])
        res = {"points": m.n, "kept": kept, "point_step": m.point_step, "message_bytes": len(data),
               "route_without": {"queued": _stat(t["without"][0]), "ready": _stat(t["without"][1])},
               "new_route": {"queued": _stat(t["new"][0]), "ready": _stat(t["new"][1])},
               "host_pass_alone": timed(host_pass),
               "decode_from_host_bytes": timed(lambda: scan.decode_msg(lay, data)),
               "decode_from_device_bytes": timed(lambda: scan.decode_msg_device(lay, d.data_ptr(), len(data))),
               "upload_bytes_route_without": 16 * kept, "upload_bytes_new_route": len(data),
               "device_bytes_model_per_point": round(m.point_step + 16 * kept / m.n, 2),
               "device_bytes_model": m.point_step * m.n + 16 * kept}
        res["ratio_ready_without_over_new"] = round(res["route_without"]["ready"]["median_ms"] / res["new_route"]["ready"]["median_ms"], 2)
        # racing mode: the layers are two legal orders of the same scans -- the same blocks, not the same bits
        a, b = (l.download() for l in layers)
        res["same_blocks_in_both_layers"] = bool({tuple(x) for x in a[0]} == {tuple(x) for x in b[0]})
        out[name] = res
        for h in integ + layers:
            h.destroy()
    print(json.dumps(out))
    scan.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
