"""The projected map (vgx_tsdf_layer_merge_submaps, cblox getProjectedMap) on a BASELINE-config-3-shaped collection:
200 city submaps at 256^3 voxels (0.2 m, 20 x 10 grid, 50 % / 67 % overlap, yaw +-0.1), raw TSDF layers kept (8 B per
voxel: 26.8 GB of sources).  Prints one JSON line: ms per projected map (host clock around the call, which returns
after its last kernel), the layer's blocks, and the byte count of profiles/projected_map.txt.

    python profiles/projected_map_bench.py [--submaps 200] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
    gw, gh = args.grid
    rng = np.random.default_rng(args.seed)
    extent = np.array(args.block_dims) * 16 * args.voxel_size
    poses = [[i * extent[0] * 0.5, j * extent[1] / 3.0, 0.0, rng.uniform(-0.1, 0.1)] for j in range(gh) for i in range(gw)]
    ctx = capi.Context(0)
    subs = []
    t0 = time.time()
    for k, p in enumerate(poses):
        subs.append(capi.Submap.synth_city(ctx, k, args.voxel_size, 16, args.block_min, args.block_dims, 0.6, 2.0, 10.0,
                                           np.array(p), args.seed))
    ctx.synchronize()
    setup_s = time.time() - t0
    T = np.array([[np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]] for p in poses], np.float32)
    layer = capi.TsdfLayer(ctx, args.voxel_size, 16)
    for _ in range(args.warmup):
        capi.projected_map(ctx, subs, T, layer)
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        capi.projected_map(ctx, subs, T, layer)       # returns once the merge kernel has finished
        times.append((time.perf_counter() - t) * 1e3)
    n_blocks, _ = layer.stats()
    vox = 16 ** 3
    src_blocks = sum(s.num_blocks() for s in subs)
    # counted bytes: every source block read once (8 B per voxel: distance + weight) -- an upper bound on the distinct
    # source bytes of the contributing pairs -- and every target block written at 12 B per voxel (the layer is empty,
    # so nothing existing is read)
    src_bytes = src_blocks * vox * 8
    out_bytes = n_blocks * vox * 12
    best = min(times)
    print(json.dumps({"workload": f"projected map, {len(subs)} city submaps @ "
                                  f"{args.block_dims[0] * 16}x{args.block_dims[1] * 16}x{args.block_dims[2] * 16}",
                      "setup_s": round(setup_s, 1), "ms_per_map": [round(x, 2) for x in times], "ms_best": round(best, 2),
                      "layer_blocks": n_blocks, "source_blocks": src_blocks, "source_bytes": src_bytes,
                      "target_bytes": out_bytes, "bytes_counted": src_bytes + out_bytes,
                      "tb_per_s_at_best": round((src_bytes + out_bytes) / (best * 1e-3) / 1e12, 3),
                      "fraction_of_8_tb_s": round((src_bytes + out_bytes) / (best * 1e-3) / 8e12, 3)}))
    layer.destroy()
    for s in subs:
        s.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
