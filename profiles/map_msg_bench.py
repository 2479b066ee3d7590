"""From "layer on the device" to "block words in host memory", with and without the map-message calls.  Prints one JSON
line; host clock, median of --reps after warm-up, the two routes alternating so that both see the same machine:

  route without  vgx_tsdf_layer_download / vgx_submap_download_layers (three or four arrays), then a plain single-thread
                 C++ interleave into block words (profiles/map_msg_host_interleave.cpp, g++ -O2) -- what a caller has to
                 do without the map-message calls
  new route      vgx_tsdf_layer_serialize / vgx_submap_serialize_layer, then vgx_map_msg_download of the words
  also           the serialise call alone (kernel, block-index copy, synchronisations) and the host interleave alone;
                 the device-to-host copy is common to both routes
Inputs: the projected map of a --grid of 256^3 city submaps (bench.py's scene: 0.2 m, 50 % / 67 % overlap, yaw +-0.1) and
one dense 256^3 city submap (TSDF alone, and TSDF + ESDF).  Both routes' words are compared.

    python profiles/map_msg_bench.py [--grid 20 10] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/map_msg_bench.py --profile-only"""
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

F = np.float32
VP = C.c_void_p


def _stat(times):
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}


def _host_pass(tmp):
    lib = os.path.join(tmp, "libmap_msg_host_interleave.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", os.path.join(ROOT, "profiles", "map_msg_host_interleave.cpp"),
                           "-o", lib])
    dll = C.CDLL(lib)
    dll.interleave_tsdf.argtypes = [VP, VP, VP, C.c_int64, VP]
    dll.interleave_esdf.argtypes = [VP, VP, C.c_int64, VP]
    dll.interleave_tsdf.restype = dll.interleave_esdf.restype = None
    return dll


def _alternate(routes, reps, warmup=2):
    t = {k: [] for k in routes}
    for k in range(warmup + reps):
        for key, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            if k >= warmup:
                t[key].append((time.perf_counter() - t0) * 1e3)
    return {k: _stat(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[20, 10])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--profile-only", action="store_true", help="10 serialisations per input and nothing else (for rocprofv3)")
    args = ap.parse_args()
    vs, vps, nv = 0.2, 16, 4096
    dims, bmin = [16, 16, 16], [-8, -8, -4]
    rng = np.random.default_rng(args.seed)
    extent = np.array(dims) * 16 * vs
    poses = [[i * extent[0] * 0.5, j * extent[1] / 3.0, 0.0, rng.uniform(-0.1, 0.1)] for j in range(args.grid[1]) for i in range(args.grid[0])]
    ctx = capi.Context(0)
    subs = [capi.Submap.synth_city(ctx, k, vs, 16, bmin, dims, 0.6, 2.0, 10.0, np.array(p), args.seed) for k, p in enumerate(poses)]
    T = np.array([[np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]] for p in poses], F)
    layer = capi.TsdfLayer(ctx, vs, 16)
    capi.projected_map(ctx, subs, T, layer)
    for s in subs[1:]:
        s.destroy()
    sm = subs[0]
    msg = capi.MapMsg(ctx)
    if args.profile_only:
        for _ in range(10):
            layer.serialize(msg)
            sm.serialize_layer("tsdf", msg)
            sm.serialize_layer("esdf", msg)
        return
    dll = _host_pass(tempfile.mkdtemp())
    out = {"reps": args.reps, "grid": args.grid}

    # 1. the projected map
    nb = layer.stats()[0]
    words_old, words_new = np.zeros((nb, nv * 3), np.uint32), np.zeros((nb, nv * 3), np.uint32)
    bi = np.zeros((nb, 3), np.int32)
    d, w, rgba = np.zeros((nb, nv), F), np.zeros((nb, nv), F), np.zeros((nb, nv, 4), np.uint8)

    def without():
        ctx.check(ctx.lib.vgx_tsdf_layer_download(layer.h, capi._ptr(bi, capi.i32p), capi._ptr(d, capi.f32p), capi._ptr(w, capi.f32p),
                                                  capi._ptr(rgba, capi.u8p)))
        dll.interleave_tsdf(d.ctypes.data, w.ctypes.data, rgba.ctypes.data, nb * nv, words_old.ctypes.data)

    def new():
        layer.serialize(msg)
        ctx.check(ctx.lib.vgx_map_msg_download(msg.h, capi._ptr(bi, capi.i32p), VP(words_new.ctypes.data)))

    res = _alternate({"route_without": without, "new_route": new}, args.reps)
    res.update(_alternate({"serialize_alone": lambda: layer.serialize(msg),
                           "host_interleave_alone": lambda: dll.interleave_tsdf(d.ctypes.data, w.ctypes.data, rgba.ctypes.data, nb * nv,
                                                                                words_old.ctypes.data)}, args.reps))
    res.update(blocks=nb, voxels=nb * nv, word_bytes=int(words_new.nbytes), same_words=bool(np.array_equal(words_old, words_new)),
               ratio_without_over_new=round(res["route_without"]["median_ms"] / res["new_route"]["median_ms"], 2))
    out["projected_map"] = res
    del words_old, words_new, d, w, rgba

    # 2. one dense 256^3 submap: TSDF alone, TSDF + ESDF
    nb = sm.num_blocks()
    td, tw, ed, eo = (np.zeros((nb, nv), t) for t in (F, F, F, np.uint8))
    tw_old, tw_new = np.zeros((nb, nv * 3), np.uint32), np.zeros((nb, nv * 3), np.uint32)
    ew_old, ew_new = np.zeros((nb, nv * 2), np.uint32), np.zeros((nb, nv * 2), np.uint32)
    p = capi._ptr
    for name, esdf in (("submap_tsdf", False), ("submap_tsdf_esdf", True)):
        def without():
            ctx.check(ctx.lib.vgx_submap_download_layers(sm.h, p(td, capi.f32p), p(tw, capi.f32p), p(ed, capi.f32p) if esdf else None,
                                                         p(eo, capi.u8p) if esdf else None))
            dll.interleave_tsdf(td.ctypes.data, tw.ctypes.data, None, nb * nv, tw_old.ctypes.data)
            if esdf:
                dll.interleave_esdf(ed.ctypes.data, eo.ctypes.data, nb * nv, ew_old.ctypes.data)

        def new():
            sm.serialize_layer("tsdf", msg)
            ctx.check(ctx.lib.vgx_map_msg_download(msg.h, None, VP(tw_new.ctypes.data)))
            if esdf:
                sm.serialize_layer("esdf", msg)
                ctx.check(ctx.lib.vgx_map_msg_download(msg.h, None, VP(ew_new.ctypes.data)))

        res = _alternate({"route_without": without, "new_route": new}, args.reps)
        res.update(_alternate({"serialize_alone": lambda: (sm.serialize_layer("tsdf", msg), esdf and sm.serialize_layer("esdf", msg))},
                              args.reps))
        res.update(blocks=nb, voxels=nb * nv, word_bytes=int(tw_new.nbytes + (ew_new.nbytes if esdf else 0)),
                   same_words=bool(np.array_equal(tw_old, tw_new) and (not esdf or np.array_equal(ew_old, ew_new))),
                   ratio_without_over_new=round(res["route_without"]["median_ms"] / res["new_route"]["median_ms"], 2))
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
