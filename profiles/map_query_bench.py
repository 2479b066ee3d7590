"""Map queries (vgx_submap_query_device: voxblox EsdfMap lookups) on one 256^3 city submap (0.1 m, vps 16), 10^7 points,
near-surface and uniform.  Four modes on the ESDF layer: nearest, interpolated, interpolated + gradient, the same with a
pose.  Device events around each call after warm-up; ms per call and G queries/s; bytes per query from the layout and
the share of 8 TB/s they imply.  Also the host path a query replaces: downloading the layers plus the numpy restatement
(tests/map_query_ref.py, on a 10^5-point subset), and -- when VGX_LIB names a build with -DVGX_QUERY_GENERIC_ROUTE
(make SUFFIX=_generic EXTRA=-DVGX_QUERY_GENERIC_ROUTE) -- the same run with the generic route alone (run both and
compare the interpolated-gradient rows).  Prints one JSON line.

    python profiles/map_query_bench.py [--n 10000000] [--reps 10]
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

F = np.float32


def bytes_per_query(mode, points_in=12):
    """the layout read: per interpolation 8 neighbours x (4 B distance + 1 B observed) + 8 LUT words (4 B); nearest: one
    voxel + one LUT word; the gradient's window route reads 32 cells and 8 LUT words for its 7 interpolations (the
    generic route 7 x 8).  Plus the point (12 B) and the outputs (4 B distance, 1 B valid, 12 B gradient).  An upper
    count of distinct bytes: neighbours share cache lines, so HBM traffic is below it."""
    cell, lut = 5, 4
    if mode == "nearest":
        rd = cell + lut
        out = 5
    elif mode == "interp":
        rd = 8 * (cell + lut)
        out = 5
    else:
        rd = 32 * cell + 8 * lut
        out = 17
    return points_in + rd + out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-n", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    import torch
    from oracle import synth
    from tests import map_query_ref as R

    vs, vps = 0.1, 16
    ctx = capi.Context(0)
    sm = capi.Submap.synth_city(ctx, 0, vs, vps, (-8, -8, -8), (16, 16, 16), 0.3, 2.0, 10.0, np.array([0.0, 0.0, 0.0, 0.1]),
                                args.seed)
    rng = np.random.default_rng(args.seed)
    assert sm.extract_isosurface_points() > 0
    iso = sm.download_points(capi.POINTS_ISOSURFACE)[0]
    near = (iso[rng.integers(0, len(iso), args.n)] + rng.normal(0, 0.05, (args.n, 3))).astype(F)
    uniform = rng.uniform(-12.8, 12.8, (args.n, 3)).astype(F)
    pose = np.array([np.cos(0.2), 0, 0, np.sin(0.2), 0.3, -0.2, 0.05], F)
    modes = [("nearest", False, False, None), ("interp", True, False, None), ("interp+grad", True, True, None),
             ("interp+grad+pose", True, True, pose)]
    st = torch.cuda.ExternalStream(ctx.get_stream()) if ctx.get_stream() else torch.cuda.default_stream()
    res = {"n": args.n, "submap_voxels": int(sm.num_blocks()) * vps ** 3, "library": os.path.basename(capi.LIB_PATH),
           "rows": []}
    for name, pts in (("near_surface", near), ("uniform", uniform)):
        tp = torch.from_numpy(pts).to("cuda:0")
        for mode, interp, grad, T in modes:
            for _ in range(3):
                sm.query_device(tp, "esdf", interp, grad, T)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(args.reps):
                e0.record(st)
                out = sm.query_device(tp, "esdf", interp, grad, T, sync=False)
                e1.record(st)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            b = bytes_per_query("nearest" if not interp else ("interp" if not grad else "grad"))
            res["rows"].append({"points": name, "mode": mode, "ms": [round(x, 4) for x in ms], "ms_median": round(med, 4),
                                "gq_per_s": round(args.n / med / 1e6, 3), "bytes_per_query": b,
                                "share_of_8TBps": round(args.n * b / (med * 1e-3) / 8e12, 4),
                                "valid": round(float(out.valid.float().mean().item()), 4)})
        del tp
    # the host path a query replaces: the raw layers downloaded, then the numpy restatement
    t = time.perf_counter()
    td, tw, ed, eo = sm.download_layers(vps)
    t_dl = (time.perf_counter() - t) * 1e3
    d = synth.SubmapData(float(F(vs)), vps, sm.block_index(), td, tw, ed, eo, np.zeros(4))
    sub = near[: args.ref_n]
    t = time.perf_counter()
    R.query(d, sub, "esdf", interpolate=True, gradient=True)
    t_ref = (time.perf_counter() - t) * 1e3
    res["host_path"] = {"download_ms": round(t_dl, 2), "layer_bytes": int(td.nbytes + tw.nbytes + ed.nbytes + eo.nbytes),
                        "numpy_interp_grad_ms": round(t_ref, 1), "numpy_points": args.ref_n,
                        "numpy_ms_per_1e7": round(t_ref * args.n / args.ref_n, 0)}
    sm.destroy()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
