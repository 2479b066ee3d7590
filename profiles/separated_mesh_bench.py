"""The separated mesh (vgx_submaps_generate_separated_mesh: cblox generateSeparatedMesh) on the BASELINE-config-3-shaped
collection of profiles/projected_map_bench.py: 200 city submaps at 256^3 voxels (0.2 m, vps 16, 20 x 10 grid, 50 % / 67 %
overlap, yaw +-0.1), raw layers kept.  Prints one JSON line: ms per separated mesh into one reused handle (host clock
around the call, which returns with the mesh complete), the same map done the old way (n x vgx_submap_generate_mesh,
each downloaded, then transformed and coloured on the host in numpy), entries, unique blocks, triangles, and the roofline
of profiles/separated_mesh.txt (8 B per staged voxel read, 52 B per triangle written, against 8 TB/s).

    python profiles/separated_mesh_bench.py [--reps 5] [--loop-reps 1]
Kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (--loop-reps 0 there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxgraph_amd import capi  # noqa: E402


def quat_rotate(q, v):
    """Eigen _transformVector in f32 (the kernel's formula)"""
    w, x, y, z = (np.float32(c) for c in q)
    u0, u1, u2 = y * v[:, 2] - z * v[:, 1], z * v[:, 0] - x * v[:, 2], x * v[:, 1] - y * v[:, 0]
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    return np.stack([(v[:, 0] + w * u0) + (y * u2 - z * u1), (v[:, 1] + w * u1) + (z * u0 - x * u2),
                     (v[:, 2] + w * u2) + (x * u1 - y * u0)], -1)


def old_way(subs, T, rgba, mesh):
    """per submap: vgx_submap_generate_mesh, download, transform and colour on the host"""
    out = []
    for s, Ts, c in zip(subs, T, rgba):
        s.generate_mesh(mesh)
        bi, first, v, n = mesh.download()
        v = quat_rotate(Ts[:4], v.reshape(-1, 3)) + Ts[4:]
        n = quat_rotate(Ts[:4], n)
        out.append((bi, first, v, n, np.broadcast_to(c, (len(n), 4))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
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
    for _ in range(args.warmup):
        mesh.generate_separated(subs, T, rgba)
    sep_ms = []
    for _ in range(args.reps):
        t = time.perf_counter()
        mesh.generate_separated(subs, T, rgba)
        sep_ms.append((time.perf_counter() - t) * 1e3)
    n_blocks, n_tris = mesh.stats()
    entries = sum(s.num_blocks() for s in subs)
    loop_ms = []
    if args.loop_reps > 0:
        one = capi.Mesh(ctx)
        old_way(subs[:2], T[:2], rgba[:2], one)                  # (warm)
        for _ in range(args.loop_reps):
            t = time.perf_counter()
            parts = old_way(subs, T, rgba, one)
            loop_ms.append((time.perf_counter() - t) * 1e3)
        assert sum(len(p[3]) for p in parts) == n_tris
        one.destroy()
    # counted bytes: every staged voxel read once (8 B: f32 distance + f32 weight; the neighbours' planes are re-reads,
    # mostly from cache) and every triangle written once (36 B vertices + 12 B normal + 4 B colour)
    read_b = entries * 16 ** 3 * 8
    write_b = n_tris * 52
    best = min(sep_ms)
    print(json.dumps({"workload": f"separated mesh, {len(subs)} city submaps @ "
                                  f"{args.block_dims[0] * 16}x{args.block_dims[1] * 16}x{args.block_dims[2] * 16}",
                      "ms_separated": [round(x, 3) for x in sep_ms], "ms_separated_best": round(best, 3),
                      "ms_per_submap_loop": [round(x, 1) for x in loop_ms],
                      "entries": entries, "unique_blocks": n_blocks, "triangles": n_tris,
                      "read_bytes": read_b, "write_bytes": write_b,
                      "floor_ms_at_8_tb_s": round((read_b + write_b) / 8e12 * 1e3, 3),
                      "fraction_of_8_tb_s": round((read_b + write_b) / (best * 1e-3) / 8e12, 3)}))
    mesh.destroy()
    for s in subs:
        s.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
