"""The connected mesh (vgx_mesh_connect: voxblox createConnectedMesh) on the BASELINE-config-3-shaped collection of
profiles/projected_map_bench.py: 200 city submaps at 256^3 voxels (0.2 m, vps 16, 20 x 10 grid, 50 % / 67 % overlap, yaw
+-0.1).  The combined mesh and the separated mesh, each welded at 1e-10f and at 0.5 * voxel_size into one reused handle,
warm.  Prints one JSON line per case: ms per call (host clock around the call, which returns with the mesh complete), ms
of the connected mesh's download, V, V / 3T, table slots, extra device bytes, the roofline's byte count (36 B per triangle
read, 12 B of indices per triangle and 28 B per unique vertex written, the table: 4 B per slot cleared, 4 B per vertex
probed twice, 8 B per vertex of rep / number written and read) and the fraction of 8 TB/s; the PLY sizes before
(vgx_mesh_write_ply) and after, from the two stated formats; and, with --host-weld, what a caller does today: vgx_mesh_download
of the soup, then a single-thread std::unordered_map weld (the helper below, compiled by this script).

    python profiles/connected_mesh_bench.py [--reps 5] [--host-weld] [--only separated]
Kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (without --host-weld)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxgraph_amd import capi  # noqa: E402

HOST_WELD = r"""
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>
struct Key { int64_t k[3]; bool operator==(const Key& o) const { return k[0] == o.k[0] && k[1] == o.k[1] && k[2] == o.k[2]; } };
struct Hash {  // voxblox's LongIndexHash [recalled]: the three coordinates times large primes
  size_t operator()(const Key& a) const { return (size_t)(a.k[0] + a.k[1] * 17191 + a.k[2] * 17191 * 17191); }
};
// createConnectedMesh over a soup: vertices [n][3] -> unique [V][3] (first occurrence), normals, indices; returns V
extern "C" int64_t host_weld(const float* v, const float* tri_normals, int64_t n, float threshold, float* out_v, float* out_n,
                             uint32_t* indices) {
  const double inv = 1.0 / (double)threshold;
  std::unordered_map<Key, uint32_t, Hash> uniques;
  int64_t nv = 0;
  for (int64_t j = 0; j < n; ++j) {
    Key key;
    for (int a = 0; a < 3; ++a) key.k[a] = (int64_t)std::round((double)v[3 * j + a] * inv);
    auto it = uniques.find(key);
    if (it == uniques.end()) {
      uniques.emplace(key, (uint32_t)nv);
      for (int a = 0; a < 3; ++a) {
        out_v[3 * nv + a] = v[3 * j + a];
        out_n[3 * nv + a] = tri_normals[3 * (j / 3) + a];
      }
      indices[j] = (uint32_t)nv++;
    } else {
      indices[j] = it->second;
    }
  }
  return nv;
}
"""


def build_host_weld(tmp):
    src, lib = os.path.join(tmp, "host_weld.cpp"), os.path.join(tmp, "libhost_weld.so")
    with open(src, "w") as f:
        f.write(HOST_WELD)
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", src, "-o", lib])
    fn = C.CDLL(lib).host_weld
    fn.restype = C.c_int64
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    fn.argtypes = [f32p, f32p, C.c_int64, C.c_float, f32p, f32p, u32p]
    return lambda v, n, thr, ov, on, idx: fn(v.ctypes.data_as(f32p), n.ctypes.data_as(f32p), v.size // 3, C.c_float(thr),
                                            ov.ctypes.data_as(f32p), on.ctypes.data_as(f32p), idx.ctypes.data_as(u32p))


def ply_bytes(n_vertices, n_faces, colored):
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\n%selement face %d\nproperty list uchar int vertex_indices\n"
              "end_header\n") % (n_vertices, "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
                                 if colored else "", n_faces)
    return len(header) + n_vertices * (28 if colored else 24) + n_faces * 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--block-dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--block-min", type=int, nargs=3, default=[-8, -8, -4])
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-weld", action="store_true")
    ap.add_argument("--only", choices=["combined", "separated"], default=None)
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
    out = capi.ConnectedMesh(ctx)
    layer = capi.TsdfLayer(ctx, args.voxel_size, 16)
    weld = None
    tmp = tempfile.TemporaryDirectory()
    if args.host_weld:
        weld = build_host_weld(tmp.name)
    for which in ("combined", "separated"):
        if args.only and which != args.only:
            continue
        if which == "combined":
            capi.combined_mesh(ctx, subs, T, layer, mesh)
        else:
            mesh.generate_separated(subs, T, rgba)
        _, n_tris = mesh.stats()
        colored = mesh.has_colors()
        n = 3 * n_tris
        for thr in (np.float32(1e-10), np.float32(0.5) * np.float32(args.voxel_size)):
            for _ in range(args.warmup):
                mesh.connect(thr, out)
            ms = []
            for _ in range(args.reps):
                t = time.perf_counter()
                mesh.connect(thr, out)
                ms.append((time.perf_counter() - t) * 1e3)
            nv, nt, _ = out.stats()
            t = time.perf_counter()
            got = out.download()
            dl_ms = (time.perf_counter() - t) * 1e3
            slots = 1024
            while slots < 2 * n:
                slots *= 2
            # the library's scratch at this size without its quarter of slack: table, rep, number (indices are output)
            extra = 4 * slots + 8 * n
            table_traffic = 4 * slots + 2 * 4 * n + 2 * 8 * n
            bytes_ = 36 * n_tris + 12 * n_tris + 28 * nv + table_traffic
            best = min(ms)
            rec = {"mesh": which, "threshold": float(thr), "triangles": n_tris, "soup_vertices": n, "V": nv,
                   "V_over_3T": round(nv / n, 4), "ms_connect": [round(x, 3) for x in ms], "ms_connect_best": round(best, 3),
                   "ms_download_connected": round(dl_ms, 1), "table_slots": slots, "extra_device_bytes": extra,
                   "roofline_bytes": bytes_, "floor_ms_at_8_tb_s": round(bytes_ / 8e12 * 1e3, 3),
                   "fraction_of_8_tb_s": round(bytes_ / (best * 1e-3) / 8e12, 4),
                   "ply_bytes_soup": ply_bytes(n, n_tris, colored), "ply_bytes_connected": ply_bytes(nv, nt, colored)}
            if weld is not None and thr == np.float32(1e-10):
                print(f"host route: {which} mesh, {n} soup vertices ...", file=sys.stderr, flush=True)
                t = time.perf_counter()
                _, _, v, nrm = mesh.download()
                soup_ms = (time.perf_counter() - t) * 1e3
                ov, on = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
                idx = np.empty(n, np.uint32)
                t = time.perf_counter()
                hv = weld(v, nrm, float(thr), ov, on, idx)
                weld_ms = (time.perf_counter() - t) * 1e3
                same = (hv == nv and np.array_equal(ov[:hv].view(np.uint32), got[0].view(np.uint32))
                        and np.array_equal(idx.reshape(-1, 3), got[3]))
                rec.update({"ms_soup_download": round(soup_ms, 1), "ms_host_weld": round(weld_ms, 1),
                            "host_route_ms": round(soup_ms + weld_ms, 1), "device_route_ms": round(best + dl_ms, 1),
                            "host_over_device": round((soup_ms + weld_ms) / (best + dl_ms), 2), "host_equals_device": bool(same)})
                del v, nrm, ov, on, idx
            del got
            print(json.dumps(rec), flush=True)
    tmp.cleanup()
    out.destroy()
    mesh.destroy()
    layer.destroy()
    for s in subs:
        s.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
