"""The depth-image decode against the route a depth camera's frame took before it: depth_image_proc's cloud through the
PointCloud2 decode.  Both fill the same vgx_scan with the same points (checked before anything is timed); what differs is
the bytes that cross the pinned stage and what the kernel reads.

  depth_host / depth_device   vgx_scan_decode_depth_image / _device: the frame's bytes in host memory (upload included) /
                              already in device memory (the kernel, its launch and the read-back alone)
  cloud_host / cloud_device   vgx_scan_decode_msg / _device of the equivalent cloud: the frame unprojected by the numpy
                              restatement, dropped pixels NaN, 16-byte pcl::PointXYZ without colours, 32-byte
                              pcl::PointXYZRGB with them

NOT timed: the host-side unprojection that builds the cloud (depth_image_proc's work), which the depth route's user no
longer runs at all.  Frames: a camera inside the room of tests/scan_msg_scenes.py at 640 x 480 and 1280 x 720, 16UC1 and
32FC1, without colours and with a registered RGB8 image.  Host clock around calls that end in a synchronisation; 10
warm-up rounds, then --reps timed rounds with the four routes alternating in one process so that all see the same
machine; median, and the 10th / 90th percentile, minimum and maximum as the spread.  One JSON line per case, then a table.

    python profiles/depth_image_decode.py [--reps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import depth_image_ref as D  # noqa: E402
from tests import scan_msg_scenes as S  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

F = np.float32
WARMUP = 10


def _stat(times):
    q = np.percentile(times, [10, 50, 90])
    return {"median_ms": round(float(q[1]), 4), "p10_ms": round(float(q[0]), 4), "p90_ms": round(float(q[2]), 4),
            "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def _cloud(img, cam, points, rgba):
    """the frame as depth_image_proc publishes it: an organised cloud with NaN where there is no depth"""
    name = "xyz16" if rgba is None else "xyzrgb32"
    m = S.Msg(img.width, img.height, S.STEP[name], S.FIELDS[name])
    packed = None
    if rgba is not None:                                                   # PCL's packed 0xAARRGGBB: bytes b g r a
        packed = (rgba[:, 2].astype(np.uint32) | (rgba[:, 1].astype(np.uint32) << 8) | (rgba[:, 0].astype(np.uint32) << 16) |
                  (rgba[:, 3].astype(np.uint32) << 24))
    return m.fill(np.random.default_rng(1), points, packed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    ctx = capi.Context(0)
    scan = capi.Scan(ctx)
    lib, C = ctx.lib, capi.C
    rows = []
    for width, height in ((640, 480), (1280, 720)):
        for encoding, ename in ((D.DEPTH_16UC1, "16UC1"), (D.DEPTH_32FC1, "32FC1")):
            for kind, cname in ((D.COLOR_NONE, "none"), (D.COLOR_RGB8, "rgb8")):
                img, cam = D.room_frame(width, height, encoding, seed=width, color_kind=kind, row_pad=0, color_pad=0)
                pts, reason, u, v = D.unproject(img, cam)
                every = D.colours(img, u, v) if kind != D.COLOR_NONE else None
                m = _cloud(img, cam, pts, every)
                lay, camera, mlay = img.layout(capi), cam.capi(capi), m.layout(capi)
                depth, cloud = np.ascontiguousarray(img.depth), np.ascontiguousarray(m.data)
                color = np.ascontiguousarray(img.color) if img.color is not None else None
                # both routes give the restatement's scan
                want = D.decode(img, cam)
                for got in (scan.decode_depth_image(lay, camera, depth, color), scan.decode_msg(mlay, cloud)):
                    have = scan.download()
                    assert got == (len(want[0]), D.dropped(want[3]))
                    assert np.array_equal(have[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(have[1], want[1])
                d_depth, d_cloud = torch.from_numpy(depth).cuda(), torch.from_numpy(cloud).cuda()
                d_color = torch.from_numpy(color).cuda() if color is not None else None
                torch.cuda.synchronize()
                cp, cn = (color.ctypes.data, len(color)) if color is not None else (None, 0)
                dcp = d_color.data_ptr() if color is not None else None
                routes = {
                    "depth_host": lambda: lib.vgx_scan_decode_depth_image(scan.h, C.byref(lay), C.byref(camera), None, depth.ctypes.data,
                                                                          len(depth), cp, cn),
                    "cloud_host": lambda: lib.vgx_scan_decode_msg(scan.h, C.byref(mlay), None, cloud.ctypes.data, len(cloud)),
                    "depth_device": lambda: lib.vgx_scan_decode_depth_image_device(scan.h, C.byref(lay), C.byref(camera), None,
                                                                                   d_depth.data_ptr(), len(depth), dcp, cn),
                    "cloud_device": lambda: lib.vgx_scan_decode_msg_device(scan.h, C.byref(mlay), None, d_cloud.data_ptr(), len(cloud)),
                }
                t = {k: [] for k in routes}
                for k in range(WARMUP + args.reps):
                    for key, fn in routes.items():
                        t0 = time.perf_counter()
                        rc = fn()
                        dt = time.perf_counter() - t0
                        assert rc == 0
                        if k >= WARMUP:
                            t[key].append(dt * 1e3)
                res = {"frame": f"{width}x{height}", "encoding": ename, "colour": cname, "reps": args.reps, "candidates": width * height,
                       "kept": len(want[0]), "depth_route_bytes": len(depth) + cn, "cloud_route_bytes": len(cloud)}
                res.update({key: _stat(v) for key, v in t.items()})
                res["host_cloud_over_depth"] = round(res["cloud_host"]["median_ms"] / res["depth_host"]["median_ms"], 2)
                res["device_cloud_over_depth"] = round(res["cloud_device"]["median_ms"] / res["depth_device"]["median_ms"], 2)
                print(json.dumps(res), flush=True)
                rows.append(res)
    print()
    print("median ms (p10 .. p90) of %d calls; bytes are what the route uploads" % args.reps)
    print("%-9s %-6s %-5s %10s %10s  %-24s %-24s %-24s %-24s %6s %6s" % ("frame", "depth", "col", "depth B", "cloud B", "depth_host", "cloud_host",
                                                                        "depth_device", "cloud_device", "host x", "dev x"))
    for r in rows:
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (r[k]["median_ms"], r[k]["p10_ms"], r[k]["p90_ms"])
        print("%-9s %-6s %-5s %10d %10d  %-24s %-24s %-24s %-24s %6.2f %6.2f" % (
            r["frame"], r["encoding"], r["colour"], r["depth_route_bytes"], r["cloud_route_bytes"], cell("depth_host"), cell("cloud_host"),
            cell("depth_device"), cell("cloud_device"), r["host_cloud_over_depth"], r["device_cloud_over_depth"]))
    scan.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
