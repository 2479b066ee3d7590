"""The elevation map on the two scenes of profiles/planar_map_bench.py at 0.1 m voxels, max_distance_m 2 m (R = 20), bands of
0.5 m and 2 m from 0.25 m under the ground, the default step window (radius 1) and a wide one (radius 5):

  city       a 256^3 city submap's ESDF layer (vgx_submap_layer_elevation_map)
  projected  the projected map of --grid submaps (vgx_tsdf_layer_elevation_map)

Prints one JSON line.  Per scene, band and window: the call on the host clock (it ends in a device synchronise), median of
--reps after warm-up; the device time by pass from the handle's events (vgx_elevation_map_set_timing, _pass_ms: box, gather,
step row, step column + class, distance row, distance column), median; the download of all eleven arrays; measured in the
same run beside it: the planar map's call on the same source and band, and the host route the call replaces -- the layer
downloaded, then tests/elevation_map_ref.py -- timed once, and whether the two agree byte for byte.

    timeout 900 python profiles/elevation_map_bench.py [--reps 20] [--scene city|projected|both]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import elevation_map_ref as R  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

F = np.float32
Z_MIN = -0.25      # the city's ground is z = 0: both bands hold it


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(float(min(times)), 3), "max_ms": round(float(max(times)), 3)}


def _timed(call, reps, after=None):
    wall, extra = [], []
    for k in range(3 + reps):
        t = time.perf_counter()
        call()
        dt = (time.perf_counter() - t) * 1e3
        if k >= 3:
            wall.append(dt)
            if after:
                extra.append(after())
    return wall, extra


def measure(name, produce, produce_planar, host_layer, esdf, vs, vps, em, pm, bands, radii, reps):
    out = {}
    host = None
    for width in bands:
        for radius in radii:
            cfg = dict(z_min=Z_MIN, z_max=Z_MIN + width, max_distance_m=2.0, step_radius_cells=radius)
            c = capi.elevation_map_config(**cfg)
            wall, passes = _timed(lambda: produce(c, em), reps, em.pass_ms)
            t = time.perf_counter()
            got = em.download()
            t_down = (time.perf_counter() - t) * 1e3
            (x0, y0), (w, h), _, states, classes = em.stats()
            row = {"cells": w * h, "box": [x0, y0, w, h], "states_unknown_surface_hole_blocked": list(states),
                   "classes_unknown_traversable_not": list(classes), "call": _stat(wall),
                   "pass_ms_box_gather_steprow_stepclass_distrow_distcolumn": [round(float(v), 4) for v in np.median(np.array(passes), axis=0)],
                   "download_ms": round(t_down, 3)}
            if radius == radii[0]:
                pc = capi.planar_map_config(z_min=Z_MIN, z_max=Z_MIN + width, max_distance_m=2.0)
                pwall, _ = _timed(lambda: produce_planar(pc, pm), reps)
                row["planar_map_call_same_source"] = _stat(pwall)
                t = time.perf_counter()
                host = host_layer()
                t_copy = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                want = R.elevation_map(vs, vps, *host, esdf, **cfg)
                t_numpy = (time.perf_counter() - t) * 1e3
                same = (w, h) == (want.W, want.H) and all(R.same(a, getattr(want, f)) for a, f in zip(got, R.FIELDS))
                row["host_route"] = {"layer_download_ms": round(t_copy, 1), "numpy_ms": round(t_numpy, 1)}
                row["identical_to_host_route"] = bool(same)
            out[f"band_{width}m_radius_{radius}"] = row
    return {name: out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[6, 6])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="both")
    args = ap.parse_args()
    vs, vps = 0.1, 16
    ctx = capi.Context(0)
    em, pm = capi.ElevationMap(ctx), capi.PlanarMap(ctx)
    em.set_timing(True)
    out = {"workload": "elevation map, 0.1 m voxels, max_distance_m 2 m", "reps": args.reps}
    bands, radii = (0.5, 2.0), (1, 5)
    if args.scene in ("city", "both"):
        sm = capi.Submap.synth_city(ctx, 0, vs, vps, (-8, -8, -8), (16, 16, 16), 0.3, 2.0, 10.0, np.array([0.0, 0.0, 0.0, 0.1]), 7)

        def city_host():
            _, _, ed, eo = sm.download_layers(vps)
            return sm.block_index(), ed, eo

        out.update(measure("city_256_esdf", lambda c, m: sm.layer_elevation_map("esdf", c, m), lambda c, m: sm.layer_planar_map("esdf", c, m),
                           city_host, True, vs, vps, em, pm, bands, radii, args.reps))
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
        out.update(measure("projected_map", lambda c, m: layer.elevation_map(c, m), lambda c, m: layer.planar_map(c, m), layer_host, False,
                           vs, vps, em, pm, bands, radii, args.reps))
        layer.destroy()
    print(json.dumps(out))
    pm.destroy()
    em.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
