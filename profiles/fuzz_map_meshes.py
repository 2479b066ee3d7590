#!/usr/bin/env python3
"""Differential fuzzing of the map products that are meshes, against their numpy restatements (tests/*_ref.py), bit for
bit, on the scenes of profiles/fuzz_map_scene.py.  Per seed, at the drawn min_weight:
  1. the combined mesh of the projected map of the posed submaps (vgx_tsdf_layer_merge_submaps, then
     vgx_tsdf_layer_generate_mesh) and the mesh of one raw submap (vgx_submap_generate_mesh), against
     mesh_ref.generate_mesh;
  2. the separated mesh of all submaps at their poses in a shuffled array order with drawn colours, on every third seed
     with one entry twice, against separated_mesh_ref.separated_mesh;
  3. each of the three connected (vgx_mesh_connect) at two of the six drawn thresholds (1e-10, half a voxel, a voxel, a
     block, four times the scene's extent, one log-uniform in [1e-20, 10]), against connected_mesh_ref.connect: vertices,
     normals, colours, indices, V and T.  A threshold the library is specified to refuse (|v * inv| >= 2^62) must be
     refused with VGX_ERR_UNSUPPORTED and raised by the restatement too.
  4. the marker of each of the three (vgx_mesh_fill_marker) in a drawn colour mode at a drawn opacity, with a drawn
     constant colour where the mesh has none and the mode needs one (and on one case in four besides), against
     mesh_marker_ref.fill_marker: points, colours and the point count.
With COLOUR=1 (off by default; the draws above do not change: the colours come from a stream of their own) also
  5. the projected map of the same submaps carrying colours, meshed with one colour per vertex
     (vgx_tsdf_layer_generate_mesh_colored), and one raw coloured submap (vgx_submap_generate_mesh_colored): the plain
     mesh unchanged, the vertex colours against map_colour_ref.vertex_colours; each welded at one drawn threshold and
     filled into a marker in COLOR or LAMBERT_COLOR, against map_colour_ref.connect / fill_marker.
A case whose restatement gives no triangle, or a weld that welds nothing or is refused, is counted as degenerate; more
than one in five per product fails.  The slowest vgx_mesh_connect call is reported with its scene.
    SEEDS=200 FIRST=1000 python profiles/fuzz_map_meshes.py
    COLOUR=1 SEEDS=200 FIRST=3000 python profiles/fuzz_map_meshes.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32


def connect_reference(soup, thr):
    """connected_mesh_ref.connect over (vertices, normals, colors or None): the tuple, or None where it refuses"""
    from tests import connected_mesh_ref as cr
    try:
        return cr.connect(soup[0], soup[1], soup[2], thr)
    except OverflowError:
        return None


def weld_is_degenerate(want):
    """refused, no triangle, or as many vertices as soup vertices"""
    return want is None or len(want[3]) == 0 or len(want[0]) == 3 * len(want[3])


def largest_weld(want):
    """the largest number of soup vertices that share one key"""
    return int(np.bincount(want[3].ravel()).max()) if want is not None and len(want[3]) else 0


def main():
    from profiles import fuzz_map_scene as S
    from profiles.fuzz_map_layers import draw_colours
    from tests import map_colour_ref as mc
    from tests import mesh_marker_ref as kr
    from tests import mesh_ref as mr
    from tests import separated_mesh_ref as sr
    from voxgraph_amd import capi
    capi.load()
    ctx = capi.Context(0)
    n_seeds, first = int(os.environ.get("SEEDS", "100")), int(os.environ.get("FIRST", "0"))
    colour = os.environ.get("COLOUR", "0") == "1"
    deg = S.Degenerate()
    tot = dict(cases=0, blocks=0, triangles=0, welds=0, refused=0, soup=0, vertices=0, markers=0, marker_points=0, coloured=0, coloured_triangles=0, moved=0)
    modes = {}
    slowest = (0.0, None)
    heaviest = (0, None)

    def fail(sc, product, msg):
        print("MISMATCH seed", sc.seed, "product", product, "\n ", msg, "\n ", S.describe(sc))
        return 1

    out = capi.ConnectedMesh(ctx)
    mesh = capi.Mesh(ctx)
    marker = capi.MeshMarker(ctx)
    for seed in range(first, first + n_seeds):
        sc = S.draw(seed)
        mrng = np.random.default_rng([seed, 0x6D6B])                     # the markers' own stream: the scene's is not touched
        vs, vps, mw = sc.voxel_size, sc.vps, sc.min_weight
        handles = [capi.Submap(ctx, i, vs, vps, s.block_index, s.tsdf_distance, s.tsdf_weight) for i, s in enumerate(sc.subs)]
        layer = capi.TsdfLayer(ctx, vs, vps)
        layer.merge_submaps(handles, sc.poses)
        bi, d, w, _ = layer.download()
        k = seed % len(sc.subs)
        order = sc.sep_order
        products = [
            ("combined mesh", lambda: layer.generate_mesh(mesh, mw),
             lambda: mr.generate_mesh(bi, d, w, vps, vs, mw)[:4]),
            ("submap mesh", lambda: handles[k].generate_mesh(mesh, mw),
             lambda: mr.generate_mesh(sc.subs[k].block_index, sc.subs[k].tsdf_distance, sc.subs[k].tsdf_weight, vps, vs, mw)[:4]),
            ("separated mesh", lambda: mesh.generate_separated([handles[i] for i in order], sc.poses[order], sc.colors[order], mw),
             lambda: sr.separated_mesh([(sc.subs[i].block_index, sc.subs[i].tsdf_distance, sc.subs[i].tsdf_weight) for i in order],
                                       sc.poses[order], sc.colors[order], vps, vs, mw)),
        ]
        for m, (name, device, reference) in enumerate(products):
            device()
            want = reference()
            got = mesh.download() + ((mesh.download_colors(),) if mesh.has_colors() else ())
            msg = S.compare(name, got, want)
            if msg or mesh.stats() != (len(want[0]), len(want[2])):
                return fail(sc, name, msg or f"stats {mesh.stats()}, want {(len(want[0]), len(want[2]))}")
            deg.count(name, len(want[2]) == 0)
            tot["blocks"] += len(want[0])
            tot["triangles"] += len(want[2])
            soup = (want[2], want[3], want[4] if len(want) > 4 else None)
            mode, opacity = int(mrng.integers(0, 6)), float(F(mrng.uniform(0, 1)))
            needs = soup[2] is None and mode in (kr.COLOR, kr.LAMBERT_COLOR)
            const = tuple(int(c) for c in mrng.integers(0, 256, 4)) if needs or mrng.random() < 0.25 else None
            capi.fill_marker(mesh, mode, opacity, const, marker)
            what = f"{name} marker in mode {mode} at opacity {opacity!r}, constant colour {const}"
            msg = S.compare(what, marker.download(), kr.fill_marker(soup[0], soup[1], soup[2], mode, opacity, const))
            if msg or marker.stats() != (3 * len(want[2]), mode):
                return fail(sc, what, msg or f"stats {marker.stats()}, want {(3 * len(want[2]), mode)}")
            modes[mode] = modes.get(mode, 0) + 1
            tot["markers"] += 1
            tot["marker_points"] += 3 * len(want[2])
            for kind, thr in sc.thresholds[2 * m:2 * m + 2]:
                wc = connect_reference(soup, thr)
                t0 = time.perf_counter()
                try:
                    mesh.connect(thr, out)
                    refused = None
                except capi.VgxError as e:
                    refused = e.code
                dt = time.perf_counter() - t0
                what = f"{name} connected at {kind} {float(thr)!r}"
                if wc is None or refused is not None:
                    if wc is not None or refused != capi.ERR_UNSUPPORTED or out.stats() != (0, 0, False):
                        return fail(sc, what, f"library refused with {refused}, restatement {'refused' if wc is None else 'did not'}, "
                                              f"stats {out.stats()}")
                    tot["refused"] += 1
                else:
                    msg = S.compare(what, out.download(), wc)
                    if msg or out.stats() != (len(wc[0]), len(wc[3]), soup[2] is not None):
                        return fail(sc, what, msg or f"stats {out.stats()}, want V {len(wc[0])} T {len(wc[3])}")
                    tot["soup"] += 3 * len(wc[3])
                    tot["vertices"] += len(wc[0])
                    if dt > slowest[0]:
                        slowest = (dt, f"{what}, seed {seed}: {3 * len(wc[3])} soup vertices -> {len(wc[0])}, largest key {largest_weld(wc)}")
                    if largest_weld(wc) > heaviest[0]:
                        heaviest = (largest_weld(wc), f"{what}, seed {seed}: {dt * 1e3:.2f} ms")
                deg.count("connected " + name, weld_is_degenerate(wc))
                tot["welds"] += 1
        # 5. one colour per vertex
        if colour:
            rgbas = draw_colours(seed, sc.subs, vps)
            for h, c in zip(handles, rgbas):
                if c is not None:
                    h.set_colors(c)
            layer.upload(np.zeros((0, 3), np.int32), np.zeros(0, F), np.zeros(0, F))
            layer.merge_submaps(handles, sc.poses)
            cbi, cd, cw, crgba = layer.download()
            kc = next(((k + i) % len(rgbas) for i in range(len(rgbas)) if rgbas[(k + i) % len(rgbas)] is not None))
            sk = sc.subs[kc]
            cases = [("coloured combined mesh", lambda: layer.generate_mesh_colored(mesh, mw), (cbi, cd, cw, crgba)),
                     ("coloured submap mesh", lambda: handles[kc].generate_mesh_colored(mesh, mw),
                      (sk.block_index, sk.tsdf_distance, sk.tsdf_weight, rgbas[kc]))]
            for m, (name, device, (sbi, sd, sw, srgba)) in enumerate(cases):
                device()
                want = mr.generate_mesh(sbi, sd, sw, vps, vs, mw)[:4]
                wcol, moved = mc.vertex_colours(want[0], want[1], want[2], sbi, sw, srgba, vps, vs, mw)
                msg = S.compare(name, mesh.download() + (mesh.download_vertex_colors(),), want + (wcol,))
                if msg or mesh.color_layout() != capi.MESH_COLORS_PER_VERTEX:
                    return fail(sc, name, msg or f"colour layout {mesh.color_layout()}")
                deg.count(name, len(want[2]) == 0)
                tot["coloured"] += 1
                tot["coloured_triangles"] += len(want[2])
                tot["moved"] += int(moved.sum())
                mode, opacity = (kr.COLOR, kr.LAMBERT_COLOR)[int(mrng.integers(0, 2))], float(F(mrng.uniform(0, 1)))
                capi.fill_marker(mesh, mode, opacity, None, marker)
                msg = S.compare(f"{name} marker in mode {mode}", marker.download(), mc.fill_marker(want[2], want[3], wcol, mode, opacity))
                if msg:
                    return fail(sc, name, msg)
                kind, thr = sc.thresholds[int(mrng.integers(0, len(sc.thresholds)))]
                try:
                    wc = mc.connect(want[2], want[3], wcol, thr)
                except OverflowError:
                    wc = None
                try:
                    mesh.connect(thr, out)
                    refused = None
                except capi.VgxError as e:
                    refused = e.code
                what = f"{name} connected at {kind} {float(thr)!r}"
                if (wc is None) != (refused is not None):
                    return fail(sc, what, f"library refused with {refused}, restatement {'refused' if wc is None else 'did not'}")
                if wc is not None:
                    msg = S.compare(what, out.download(), wc)
                    if msg or out.stats() != (len(wc[0]), len(wc[3]), True):
                        return fail(sc, what, msg or f"stats {out.stats()}")
        layer.destroy()
        for h in handles:
            h.destroy()
        tot["cases"] += 1
    out.destroy()
    marker.destroy()
    mesh.destroy()
    ctx.close()
    over = deg.exceeded()
    print("degenerate cases per product:", {p: (deg.degenerate[p], n) for p, n in deg.cases.items()})
    print(f"slowest vgx_mesh_connect (call and synchronisation, host clock): {slowest[0] * 1e3:.2f} ms, {slowest[1]}")
    print(f"largest single key: {heaviest[0]} soup vertices, {heaviest[1]}")
    if over:
        print("TOO MANY DEGENERATE CASES (more than one in five):", over)
        return 1
    print("no mismatch:", tot["cases"], "scenes,", tot["blocks"], "mesh blocks,", tot["triangles"], "triangles,", tot["welds"],
          "welds (", tot["refused"], "refused as specified ),", tot["soup"], "soup vertices welded into", tot["vertices"], ";",
          tot["markers"], "markers,", tot["marker_points"], "points, per mode", dict(sorted(modes.items())))
    if colour:
        print("with colours:", tot["coloured"], "meshes,", tot["coloured_triangles"], "triangles,", tot["moved"],
              "vertices coloured from a neighbouring block; each welded once and filled into a COLOR / LAMBERT_COLOR marker")
    return 0


if __name__ == "__main__":
    sys.exit(main())
