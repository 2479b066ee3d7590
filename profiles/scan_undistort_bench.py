"""The undistorting scan decode against the plain decode of the same message in the same run.  Prints one JSON line; host
clock around calls that end in a synchronisation, median of --reps after 5 warm-up rounds, the routes alternating in one
process so that all see the same machine:

  plain / undistorted      vgx_scan_decode_msg / vgx_scan_decode_msg_undistorted
  from host / from device  the message's bytes in host memory (upload included) / already in device memory
  K = 1024 / K = 64        a knot at every column stamp / 64 knots evenly spaced from the first stamp to the last

Input: the 64 x 1024 driver48 LiDAR cloud of tests/scan_msg_scenes.py with column stamps in its `t` field.  The
undistorted result is compared with the restatement (tests/scan_undistort_ref.py) before anything is timed.

    python profiles/scan_undistort_bench.py [--reps 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scan_msg_scenes as S  # noqa: E402
from tests import scan_undistort_ref as U  # noqa: E402
from tests import scan_undistort_scenes as Z  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

F = np.float32
SWEEP_NS, COLS, ROWS = 100_000_000, 1024, 64


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def _track(K):
    """a sensor at 2 m/s and 1 rad/s about z over the sweep, relative to its pose at the sweep's end"""
    stamps = np.arange(COLS) * (SWEEP_NS // COLS) * 1e-9
    kt = stamps if K == COLS else np.linspace(stamps[0], stamps[-1], K)
    tr = capi.ScanTrack()
    for t in kt:
        tr.add(t, [np.cos(0.5 * t), 0, 0, np.sin(0.5 * t), 2.0 * t, 0, 0])
    end = SWEEP_NS * 1e-9
    return tr.relative_to([np.cos(0.5 * end), 0, 0, np.sin(0.5 * end), 2.0 * end, 0, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    ctx = capi.Context(0)
    scan = capi.Scan(ctx)
    m = S.lidar(1, name="driver48")
    f = U.TimeField(U.TIME_UINT32, 20, 1e-9, 0.0)
    Z.put_time(m, f, np.tile(np.arange(COLS, dtype=np.uint32) * np.uint32(SWEEP_NS // COLS), ROWS))
    lay, field = m.layout(capi), f.capi(capi)
    data = np.ascontiguousarray(m.data)
    d = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    out = {"reps": args.reps, "points": m.n, "point_step": m.point_step, "message_bytes": len(data)}
    for K in (COLS, 64):
        kt, kT = _track(K)
        want = U.decode(m, f, kt, kT)
        scan.decode_undistorted(lay, data, field, kt, kT)
        got = scan.download()
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        view, keep = capi.scan_track_view(kt, kT)
        lib, C = ctx.lib, capi.C
        routes = {
            "plain_from_host": lambda: lib.vgx_scan_decode_msg(scan.h, C.byref(lay), None, data.ctypes.data, len(data)),
            "undistorted_from_host": lambda: lib.vgx_scan_decode_msg_undistorted(scan.h, C.byref(lay), None, C.byref(field), C.byref(view),
                                                                                 data.ctypes.data, len(data)),
            "plain_from_device": lambda: lib.vgx_scan_decode_msg_device(scan.h, C.byref(lay), None, d.data_ptr(), len(data)),
            "undistorted_from_device": lambda: lib.vgx_scan_decode_msg_undistorted_device(scan.h, C.byref(lay), None, C.byref(field),
                                                                                          C.byref(view), d.data_ptr(), len(data)),
        }
        t = {k: [] for k in routes}
        for k in range(5 + args.reps):
            for key, fn in routes.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = time.perf_counter() - t0
                assert rc == 0
                if k >= 5:
                    t[key].append(dt * 1e3)
        res = {key: _stat(v) for key, v in t.items()}
        res["kept"], res["clamped"] = len(want[0]), want[3]["clamped"]
        res["track_bytes"] = len(kt) * 36
        for src in ("host", "device"):
            res[f"ratio_undistorted_over_plain_from_{src}"] = round(res[f"undistorted_from_{src}"]["median_ms"] /
                                                                    res[f"plain_from_{src}"]["median_ms"], 2)
        out[f"K_{len(kt)}"] = res
    print(json.dumps(out))
    scan.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
