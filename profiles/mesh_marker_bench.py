"""The mesh marker (vgx_mesh_fill_marker: voxblox_ros fillMarkerWithMesh) on the BASELINE-config-3-shaped collection of
profiles/projected_map_bench.py: 200 city submaps at 256^3 voxels (0.2 m, vps 16, 20 x 10 grid, 50 % / 67 % overlap, yaw
+-0.1).  The combined mesh in NORMALS and the separated mesh in LAMBERT_COLOR (voxgraph's two modes), plus the other modes
with --all-modes, each into one reused handle, warm.  Prints one JSON line per case: ms per call (host clock around the
call, which returns with the marker complete), the byte count (52 B read and 120 B written per triangle; 48 B read in the
modes that read no colour), achieved bytes/s, and the same-run device copy ceiling from the bench tooling
(vgx_bench_stream_ceiling: float4 loads of as many bytes in, float4 stores of as many bytes out) with the fraction reached.

    python profiles/mesh_marker_bench.py [--reps 5] [--all-modes] [--only separated]
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

MODE_NAMES = {capi.MARKER_COLOR: "COLOR", capi.MARKER_HEIGHT: "HEIGHT", capi.MARKER_NORMALS: "NORMALS", capi.MARKER_GRAY: "GRAY",
              capi.MARKER_LAMBERT: "LAMBERT", capi.MARKER_LAMBERT_COLOR: "LAMBERT_COLOR"}


def bytes_per_triangle(mode, colored, constant):
    """what the kernel has to move: the soup, the normals where the mode shades by them, the colours where it reads them"""
    read = 36
    if mode in (capi.MARKER_NORMALS, capi.MARKER_LAMBERT, capi.MARKER_LAMBERT_COLOR):
        read += 12
    if mode in (capi.MARKER_COLOR, capi.MARKER_LAMBERT_COLOR) and colored and not constant:
        read += 4
    return read, 120


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--all-modes", action="store_true")
    ap.add_argument("--no-ceiling", action="store_true", help="skip the copy ceiling (a kernel-trace run wants the marker kernel alone)")
    ap.add_argument("--only", choices=["combined", "separated"], default=None)
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
    import torch
    gw, gh = args.grid
    rng = np.random.default_rng(args.seed)
    extent = np.array(args.block_dims) * 16 * args.voxel_size
    poses = [[i * extent[0] * 0.5, j * extent[1] / 3.0, 0.0, rng.uniform(-0.1, 0.1)] for j in range(gh) for i in range(gw)]
    ctx = capi.Context(0)
    subs = [capi.Submap.synth_city(ctx, k, args.voxel_size, 16, args.block_min, args.block_dims, 0.6, 2.0, 10.0,
                                   np.array(p), args.seed) for k, p in enumerate(poses)]
    ctx.synchronize()
    T = np.array([[np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]] for p in poses], np.float32)
    rgba = np.stack([capi.submap_color(k) for k in range(len(subs))])
    mesh = capi.Mesh(ctx)
    out = capi.MeshMarker(ctx)
    layer = capi.TsdfLayer(ctx, args.voxel_size, 16)
    for which in ("combined", "separated"):
        if args.only and which != args.only:
            continue
        if which == "combined":
            capi.combined_mesh(ctx, subs, T, layer, mesh)
            cases = [(capi.MARKER_NORMALS, None)]
        else:
            mesh.generate_separated(subs, T, rgba)
            cases = [(capi.MARKER_LAMBERT_COLOR, None)]
        if args.all_modes:
            cases += [(m, None if which == "separated" else (200, 30, 255, 255)) for m in MODE_NAMES if m != cases[0][0]]
        _, n_tris = mesh.stats()
        colored = mesh.has_colors()
        ceiling = {}
        for mode, const in cases:
            for _ in range(args.warmup):
                capi.fill_marker(mesh, mode, 0.8, const, out)
            ms = []
            for _ in range(args.reps):
                t = time.perf_counter()
                capi.fill_marker(mesh, mode, 0.8, const, out)
                ms.append((time.perf_counter() - t) * 1e3)
            rd, wr = bytes_per_triangle(mode, colored, const is not None)
            med = float(np.median(ms))
            nbytes = (rd + wr) * n_tris
            rec = {"mesh": which, "mode": MODE_NAMES[mode], "constant_color": const is not None, "triangles": n_tris,
                   "points": out.stats()[0], "ms_fill": [round(x, 3) for x in ms], "ms_fill_median": round(med, 3),
                   "bytes_read_per_triangle": rd, "bytes_written_per_triangle": wr, "bytes": nbytes,
                   "TBs_achieved_host_clock": round(nbytes / (med * 1e-3) / 1e12, 3),
                   "floor_ms_at_8_tb_s": round(nbytes / 8e12 * 1e3, 3)}
            if not args.no_ceiling:
                if rd not in ceiling:                       # as many bytes in and out through the tooling's float4 streams
                    src = torch.empty(rd * n_tris, dtype=torch.uint8, device="cuda:0").zero_()
                    dst = torch.empty(wr * n_tris, dtype=torch.uint8, device="cuda:0").zero_()
                    torch.cuda.synchronize()
                    capi.stream_ceiling_ms(ctx, src.data_ptr(), rd * n_tris, dst.data_ptr(), wr * n_tris, 2)
                    ceiling[rd] = capi.stream_ceiling_ms(ctx, src.data_ptr(), rd * n_tris, dst.data_ptr(), wr * n_tris, 5)
                    del src, dst
                    torch.cuda.empty_cache()
                rec.update({"ms_copy_ceiling": round(ceiling[rd], 3),
                            "TBs_copy_ceiling": round(nbytes / (ceiling[rd] * 1e-3) / 1e12, 3),
                            "host_clock_fraction_of_copy_ceiling": round(ceiling[rd] / med, 3)})
            print(json.dumps(rec), flush=True)
    out.destroy()
    mesh.destroy()
    layer.destroy()
    for s in subs:
        s.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
