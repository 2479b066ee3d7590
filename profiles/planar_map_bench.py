"""The planar map on two scenes at 0.1 m voxels, max_distance_m 2 m (R = 20), bands of 0.5 m and 2 m:

  city       a 256^3 city submap's ESDF layer (vgx_submap_layer_planar_map)
  projected  the projected map of --grid submaps (vgx_tsdf_layer_planar_map)

Prints one JSON line.  Per scene and band: the call on the host clock (it ends in a device synchronise), median of --reps
after warm-up; the device time by pass from the handle's events (vgx_planar_map_set_timing, _pass_ms: box, gather, row, column), median;
the download; the host route the call replaces -- the layer downloaded, then tests/planar_map_ref.py -- timed once, and
whether the two agree byte for byte; the bytes each pass has to move and the time that takes at 8 TB/s.

    timeout 900 python profiles/planar_map_bench.py [--reps 20] [--scene city|projected|both]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import planar_map_ref as R  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

F = np.float32


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(float(min(times)), 3), "max_ms": round(float(max(times)), 3)}


def measure(name, produce, host_layer, esdf, vs, vps, pm, bands, reps, voxel_bytes):
    out = {}
    for width in bands:
        cfg = dict(z_min=0.3, z_max=0.3 + width, max_distance_m=2.0)
        c = capi.planar_map_config(**cfg)
        wall, passes = [], []
        for k in range(3 + reps):
            t = time.perf_counter()
            produce(c, pm)
            dt = (time.perf_counter() - t) * 1e3
            if k >= 3:
                wall.append(dt)
                passes.append(pm.pass_ms())
        t = time.perf_counter()
        got = pm.download()
        t_down = (time.perf_counter() - t) * 1e3
        (x0, y0), (w, h), _, counts = pm.stats()
        t = time.perf_counter()
        bi, d, seen = host_layer()
        t_copy = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        want = R.planar_map(vs, vps, bi, d, seen, esdf, **cfg)
        t_numpy = (time.perf_counter() - t) * 1e3
        same = (w, h) == (want.W, want.H) and all(R.same(a, getattr(want, f)) for a, f in
                                                  zip(got, ("state", "occupancy", "clearance", "height", "distance")))
        cells = w * h
        rows = int(((F(cfg["z_min"]) <= R.row_centres(vs, vps, bi[:, 2])) & (R.row_centres(vs, vps, bi[:, 2]) <= F(cfg["z_max"]))).sum())
        gather_bytes = rows * vps * vps * voxel_bytes + cells * 10      # the band's voxel rows read; 10 B per cell written
        p = np.median(np.array(passes), axis=0)
        out[f"band_{width}m"] = {
            "cells": cells, "box": [x0, y0, w, h], "counts_unknown_free_occupied": list(counts), "band_voxel_rows": rows,
            "call": _stat(wall), "pass_ms_box_gather_row_column": [round(float(v), 4) for v in p], "download_ms": round(t_down, 3),
            "host_route": {"layer_download_ms": round(t_copy, 1), "numpy_ms": round(t_numpy, 1)}, "identical_to_host_route": bool(same),
            "bytes": {"gather": gather_bytes, "row_pass_at_least": cells * 3, "column_pass_at_least": cells * 6},
            "gather_floor_ms_at_8_tb_s": round(gather_bytes / 8e12 * 1e3, 5),
            "gather_fraction_of_8_tb_s": round(gather_bytes / 8e12 * 1e3 / max(float(p[1]), 1e-9), 4)}
    return {name: out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[6, 6])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="both")
    args = ap.parse_args()
    vs, vps = 0.1, 16
    ctx = capi.Context(0)
    pm = capi.PlanarMap(ctx)
    pm.set_timing(True)
    out = {"workload": "planar map, 0.1 m voxels, max_distance_m 2 m", "reps": args.reps}
    bands = (0.5, 2.0)
    if args.scene in ("city", "both"):
        sm = capi.Submap.synth_city(ctx, 0, vs, vps, (-8, -8, -8), (16, 16, 16), 0.3, 2.0, 10.0, np.array([0.0, 0.0, 0.0, 0.1]), 7)

        def city_host():
            _, _, ed, eo = sm.download_layers(vps)
            return sm.block_index(), ed, eo

        out.update(measure("city_256_esdf", lambda c, m: sm.layer_planar_map("esdf", c, m), city_host, True, vs, vps, pm, bands,
                           args.reps, 5))
        sm.destroy()
    if args.scene in ("projected", "both"):
        gw, gh = args.grid
        rng = np.random.default_rng(2)
        dims = (8, 8, 8)
        extent = np.array(dims) * vps * vs
        poses = [[i * extent[0] * 0.5, j * extent[1] * 0.5, 0.0, rng.uniform(-0.1, 0.1)] for j in range(gh) for i in range(gw)]
        subs = [capi.Submap.synth_city(ctx, k, vs, vps, (-4, -4, -4), dims, 0.3, 2.0, 10.0, np.array(p), 2) for k, p in enumerate(poses)]
        T = np.array([[np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]] for p in poses], F)
        layer = capi.TsdfLayer(ctx, vs, vps)
        capi.projected_map(ctx, subs, T, layer)
        for h in subs:
            h.destroy()

        def layer_host():
            bi, d, w, _ = layer.download()
            return bi, d, w

        out["projected_submaps"] = len(poses)
        out.update(measure("projected_map", lambda c, m: layer.planar_map(c, m), layer_host, False, vs, vps, pm, bands, args.reps, 8))
        layer.destroy()
    print(json.dumps(out))
    pm.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
