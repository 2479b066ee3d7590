"""Voxel colours through the map on the BASELINE-config-3-shaped collection of
profiles/projected_map_bench.py: 200 city submaps at 256^3 voxels (0.2 m, vps 16, 20 x 10 grid, 50 % / 67 % overlap, yaw
+-0.1), warm handles, host clock around each call (every call returns with its product complete), median of --reps.
One JSON line per case:
  plain      vgx_tsdf_layer_merge_submaps with colourless submaps and vgx_tsdf_layer_generate_mesh.  --plain-only stops
             here and binds none of the colour symbols, so that VGX_LIB can point at a build of the parent commit: the
             before / after pair is this script run on both builds back to back, twice each.
  coloured   the same merge with every submap carrying colours (one 64 MiB array uploaded to each), beside the plain one,
             with the extra bytes counted: one rgba read and one write per layer voxel, and 8 gathered colour words per
             (layer voxel, submap) pair that interpolated -- the pairs are counted as the layer's voxels of weight > 0
             times the mean number of submaps over a block, an estimate.
  vertex     vgx_tsdf_layer_generate_mesh_colored beside the plain generator on the same layer: the difference is the
             vertex-colour kernel (36 B of vertices in, 12 B out per triangle, plus 3 gathered voxel words and weights),
             against the bench tooling's float4 copy ceiling for 36 B in and 12 B out per triangle, same run.

    python profiles/map_colour_bench.py [--reps 5] [--plain-only] [--no-ceiling]
Kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (--no-ceiling)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxgraph_amd import capi  # noqa: E402

COLOUR_SYMBOLS = ("vgx_submap_from_tsdf_layer_colored", "vgx_submap_set_colors", "vgx_submap_has_colors",
                  "vgx_submap_download_colors", "vgx_tsdf_layer_generate_mesh_colored", "vgx_submap_generate_mesh_colored",
                  "vgx_mesh_color_layout", "vgx_mesh_download_vertex_colors")


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def stats(ms):
    return {"ms": [round(x, 3) for x in ms], "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true", help="the colourless merge and the plain mesh only (any build)")
    ap.add_argument("--no-ceiling", action="store_true")
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
    if args.plain_only:
        for name in COLOUR_SYMBOLS:
            capi.SIGNATURES.pop(name, None)
    gw, gh = args.grid
    rng = np.random.default_rng(args.seed)
    extent = np.array(args.block_dims) * 16 * args.voxel_size
    poses = [[i * extent[0] * 0.5, j * extent[1] / 3.0, 0.0, rng.uniform(-0.1, 0.1)] for j in range(gh) for i in range(gw)]
    ctx = capi.Context(0)
    subs = [capi.Submap.synth_city(ctx, k, args.voxel_size, 16, args.block_min, args.block_dims, 0.6, 2.0, 10.0,
                                   np.array(p), args.seed) for k, p in enumerate(poses)]
    ctx.synchronize()
    T = np.array([[np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]] for p in poses], np.float32)
    layer = capi.TsdfLayer(ctx, args.voxel_size, 16)
    mesh = capi.Mesh(ctx)
    empty = (np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    build = os.environ.get("VGX_LIB") or "this tree"

    def merge():
        layer.upload(*empty)
        t = time.perf_counter()
        layer.merge_submaps(subs, T)
        merge.ms.append((time.perf_counter() - t) * 1e3)

    def merge_ms():
        merge.ms = []
        for _ in range(args.warmup + args.reps):
            merge()
        return merge.ms[args.warmup:]

    plain_merge = merge_ms()
    n_blocks = layer.stats()[0]
    print(json.dumps({"case": "plain merge", "build": build, "layer_blocks": n_blocks, **stats(plain_merge)}), flush=True)
    plain_mesh = timed(lambda: layer.generate_mesh(mesh), args.warmup, args.reps)
    n_tris = mesh.stats()[1]
    print(json.dumps({"case": "plain mesh", "build": build, "triangles": n_tris, **stats(plain_mesh)}), flush=True)
    if not args.plain_only:
        vox = 16 ** 3
        nb = subs[0].num_blocks()
        rgba = np.random.default_rng(1).integers(0, 256, (nb, vox, 4), dtype=np.uint8)
        for s in subs:
            s.set_colors(rgba)
        del rgba
        col_merge = merge_ms()
        _, _, w, _ = layer.download()
        covered = int((w > 0).sum())
        del w
        per_block = float(sum(s.num_blocks() for s in subs)) / max(n_blocks, 1)   # mean submaps over a layer block
        extra = 8 * n_blocks * vox + int(32 * covered * per_block)
        rec = {"case": "coloured merge", "layer_blocks": layer.stats()[0], **stats(col_merge),
               "plain_ms_median": round(float(np.median(plain_merge)), 3),
               "ratio_to_plain": round(float(np.median(col_merge) / np.median(plain_merge)), 3),
               "extra_bytes_rgba_read_write": 8 * n_blocks * vox, "extra_bytes_gathered_estimate": int(32 * covered * per_block),
               "extra_GBs_over_extra_time": round(extra / max((np.median(col_merge) - np.median(plain_merge)) * 1e-3, 1e-9) / 1e9, 1)}
        print(json.dumps(rec), flush=True)
        plain2 = timed(lambda: layer.generate_mesh(mesh), args.warmup, args.reps)
        col_mesh = timed(lambda: layer.generate_mesh_colored(mesh), args.warmup, args.reps)
        n_tris = mesh.stats()[1]
        kernel_ms = float(np.median(col_mesh) - np.median(plain2))
        streamed, gathered = 48 * n_tris, 24 * n_tris                                # 3 colour words + 3 weights per triangle
        rec = {"case": "vertex colours", "triangles": n_tris, "coloured_mesh": stats(col_mesh), "plain_mesh_same_layer": stats(plain2),
               "ms_difference_of_medians": round(kernel_ms, 3), "bytes_streamed": streamed, "bytes_gathered": gathered,
               "TBs_streamed_over_difference": round(streamed / max(kernel_ms * 1e-3, 1e-9) / 1e12, 3)}
        if not args.no_ceiling:
            import torch
            src = torch.empty(36 * n_tris, dtype=torch.uint8, device="cuda:0").zero_()
            dst = torch.empty(12 * n_tris, dtype=torch.uint8, device="cuda:0").zero_()
            torch.cuda.synchronize()
            capi.stream_ceiling_ms(ctx, src.data_ptr(), 36 * n_tris, dst.data_ptr(), 12 * n_tris, 2)
            ceil = capi.stream_ceiling_ms(ctx, src.data_ptr(), 36 * n_tris, dst.data_ptr(), 12 * n_tris, 5)
            rec.update({"ms_copy_ceiling": round(ceil, 3), "TBs_copy_ceiling": round(streamed / (ceil * 1e-3) / 1e12, 3),
                        "difference_over_ceiling": round(kernel_ms / ceil, 2)})
        print(json.dumps(rec), flush=True)
    mesh.destroy()
    layer.destroy()
    for s in subs:
        s.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
