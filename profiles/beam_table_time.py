"""Beam-table range images against the uniform model, per scan, from a decoded scan that is resident on the device (the
method of profiles/range_image_time.py: the street and the yaml room of DESIGN.md 31, 16 voxels a side, the same scan from
the same pose again and again, host clock around calls that end in a synchronisation, WARMUP rounds, then --reps timed
rounds with the routes alternating in one process, median with the 10th / 90th percentile):

  uniform         vgx_range_image_build (queued) + vgx_tsdf_integrate_range_image, counted: the 64-row uniform model
  table           the same through vgx_range_image_build_beams: a table that restates the uniform row centres (offsets zero,
                  the limit inf) -- the same rows, so the difference is the row search and the second wrap pass
  uniform32       a uniform 32-row model over the span of ...
  table32         ... a 32-row table, 0.33 degrees apart near the horizon and up to 9 degrees apart at the edges, with
                  azimuth offsets up to 4.2 degrees: the wide outer rows widen the candidate box

Each route sweeps ITS sensor over the scene (one return per pixel, a quarter of a column and of the row's half extent of
jitter).  The library under test is the one VGX_LIB names: two forms of the row search were compared as two side-by-side builds
(DESIGN.md 32 has the form that lost).  The uniform route against the parent commit: run
profiles/range_image_time.py --only range_image in both trees, in turn.  The kernels' own times and the launch and copy
count come from a kernel trace of --only <route>, taken in a run of its own.

    python profiles/beam_table_time.py [--reps 100] [--only table] [--scene street]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.range_image_time import POSE, ROOM, STREET, VPS, WARMUP, YAML, _clocks, _stat  # noqa: E402
from tests import beam_table_ref as B  # noqa: E402
from tests import range_image_scenes as S  # noqa: E402
from voxgraph_amd import capi  # noqa: E402

SCENES = {"street 64x1024": STREET, "room 64x1024 yaml": ROOM}
WIDTH = 1024


def sensors():
    uniform = B.Model(WIDTH, 64, float(B.PI), 1, 0.3927, -0.3927)
    gaps = np.radians(np.concatenate([[9, 7, 5, 3, 2, 1], np.full(20, 0.33), [1, 2, 3, 5, 9]]))
    el = (-0.5 * gaps.sum() + np.concatenate([[0.0], np.cumsum(gaps)]))[::-1]          # the top row first, as the uniform model
    off = np.radians(4.2) * np.sin(np.arange(32) * 2.1)
    table32 = B.BeamModel(WIDTH, el, off, float(B.PI), 1)
    return {"uniform": uniform, "table": B.uniform_as_table(uniform),
            "uniform32": B.Model(WIDTH, 32, float(B.PI), 1, float(el[0]), float(el[-1])), "table32": table32}


def sweep(model, box, seed):
    """one return per pixel from the inside of an axis-aligned box around the sensor, in the sensor frame"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(model.height), np.arange(model.width), indexing="ij")
    uj = u + rng.uniform(-0.25, 0.25, u.shape)
    if isinstance(model, B.BeamModel):
        lo, hi = model.extent(v)
        e = model.row_elevation_rad.astype(np.float64)[v]
        d = model.direction(uj, v, rng.uniform(-0.25, 0.25, u.shape) * np.minimum(e - lo, hi - e)).reshape(-1, 3)
    else:
        d = model.centre(uj, v + rng.uniform(-0.25, 0.25, v.shape)).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, box[1] / d, np.where(d < 0, box[0] / d, np.inf)).min(1)
    pts = (d * t[:, None]).astype(np.float32)
    return pts, rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--only", default="")
    ap.add_argument("--scene", default="")
    args = ap.parse_args()
    print("library:", capi.LIB_PATH)
    print("clocks before:", _clocks(), flush=True)
    ctx = capi.Context(0)
    lib, C = ctx.lib, capi.C
    Tp = POSE.ctypes.data_as(capi.f32p)
    rows = []
    for name, box in SCENES.items():
        if args.scene and args.scene not in name:
            continue
        handles, routes, info = [], {}, {}
        for key, model in sensors().items():
            if args.only and key != args.only:
                continue
            pts, rgba = sweep(model, box, WIDTH)
            data, layout = S.message(pts, rgba)
            scan = capi.Scan(ctx)
            scan.decode_msg(capi.scan_layout(**layout), data)
            layer = capi.TsdfLayer(ctx, 0.20, VPS)
            integ = capi.FastTsdfIntegrator(ctx, capi.tsdf_config(**YAML), layer)
            image = capi.RangeImage(ctx)
            handles += [image, scan, integ, layer]
            counts, cm = capi.ProjectiveCounts(), model.capi(capi)
            build = lib.vgx_range_image_build_beams if isinstance(model, B.BeamModel) else lib.vgx_range_image_build

            def route(build=build, image=image, cm=cm, scan=scan, integ=integ, counts=counts):
                rc = build(image.h, C.byref(cm), scan.h, None)
                return rc or lib.vgx_tsdf_integrate_range_image(integ.h, Tp, image.h, C.byref(counts))
            routes[key] = route
            info[key] = (layer, image, counts, len(pts))
        t = {k: [] for k in routes}
        for k in range(WARMUP + args.reps):
            for key, fn in routes.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = time.perf_counter() - t0
                assert rc == 0, (key, rc)
                if k >= WARMUP:
                    t[key].append(dt * 1e3)
        res = {"scene": name, "reps": args.reps, "voxel_size": 0.20, "vps": VPS}
        for key, (layer, image, counts, n) in info.items():
            ic = image.stats()
            res[key] = dict(_stat(t[key]), points=n, n_filled=int(ic["n_filled"]), n_collided=int(ic["n_collided"]),
                            blocks=layer.stats()[0], **{k: getattr(counts, k) for k, _ in capi.ProjectiveCounts._fields_})
        print(json.dumps(res), flush=True)
        rows.append((res, list(routes)))
        for h in handles:
            h.destroy()
    print("clocks after:", _clocks())
    print()
    print("median ms (p10 .. p90) per scan; candidate blocks")
    for res, keys in rows:
        print(res["scene"], "  ".join("%s %.3f (%.3f .. %.3f) %d" % (k, res[k]["median_ms"], res[k]["p10_ms"], res[k]["p90_ms"],
                                                                      res[k]["n_candidate_blocks"]) for k in keys))
    ctx.close()


if __name__ == "__main__":
    main()
