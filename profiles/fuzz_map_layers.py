#!/usr/bin/env python3
"""Differential fuzzing of the map products that are layers, against their numpy restatements (tests/*_ref.py), bit for
bit, on the scenes of profiles/fuzz_map_scene.py (grid-aligned poses, dyadic voxel sizes, planted validity thresholds,
block boxes far from the origin, one-block submaps and slabs).  Per seed:
  1. vgx_tsdf_layer_merge_submaps into an empty layer and into one that holds data and colours (the colours survive),
     against projected_map_ref.merge_submaps;
  2. vgx_tsdf_layer_transform_submap against map_eval_ref.transform_layer;
  3. the projected layer made a submap (vgx_submap_from_tsdf_layer, vgx_submap_generate_esdf);
  4. vgx_submap_query on it against map_query_ref.query over the downloaded layers: three drawn flag / pose / layer
     combinations, the points those of tests/test_map_query_gpu.py plus voxel centres and faces seen through the pose;
  5. vgx_evaluate_layers_rmse of it and a partly overlapping partner against map_eval_ref.evaluate_layers_rmse: every
     detail (the f64 sum by its bits) and the error layer, two drawn layer / mode combinations.
With COLOUR=1 (off by default; the draws above do not change: the colours come from a stream of their own) also
  6. the same merges and the transform with submaps that carry colours (vgx_submap_set_colors; on two seeds in three one
     drawn submap stays colourless), distance, weight and rgba against map_colour_ref.merge_submaps / transform_submap.
A case whose restatement gives an empty product is counted as degenerate; more than one in five per product fails.
    SEEDS=200 FIRST=1000 python profiles/fuzz_map_layers.py
    COLOUR=1 SEEDS=200 FIRST=3000 python profiles/fuzz_map_layers.py"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
DETAILS_INT = ("num_evaluated_voxels", "num_ignored_voxels", "num_overlapping_voxels", "num_non_overlapping_voxels")
DETAILS_F64 = ("total_squared_error", "rmse", "max_error", "min_error", "min_abs_error")


def layer_dict(bi, d, w):
    return {tuple(int(v) for v in b): (dd, ww) for b, dd, ww in zip(bi, d, w)}


def compare_details(got, want):
    for k in DETAILS_INT:
        if got[k] != want[k]:
            return f"details {k}: got {got[k]} want {want[k]}"
    for k in DETAILS_F64:
        if np.float64(got[k]).tobytes() != np.float64(want[k]).tobytes():
            return f"details {k}: got {got[k]!r} want {want[k]!r}"
    return None


def eval_reference(gt, test, layer, mode, vps):
    """map_eval_ref.evaluate_layers_rmse over two SubmapData"""
    from tests import map_eval_ref as me
    if layer == 0:
        g, t = (me.esdf_layer(s.block_index, s.esdf_distance, s.esdf_observed) for s in (gt, test))
    else:
        g, t = (me.tsdf_layer(s.block_index, s.tsdf_distance, s.tsdf_weight) for s in (gt, test))
    return me.evaluate_layers_rmse(g, t, mode, vps)


def draw_colours(seed, subs, vps):
    """COLOUR=1: per submap [n][vps^3][4] u8 from a stream of its own -- four distinct bytes per voxel, three voxels in ten
    all 0 / 255 (where the clamp of the interpolated channel is reached) -- or None for the submap left colourless"""
    crng = np.random.default_rng([seed, 0x636F])
    out = []
    for s in subs:
        n = len(s.block_index)
        c = crng.integers(0, 256, (n, vps ** 3, 4), dtype=np.uint8)
        slab = crng.random((n, vps ** 3)) < 0.3
        c[slab] = crng.choice(np.array([0, 255], np.uint8), (int(slab.sum()), 4))
        out.append(c)
    if seed % 3 and len(out) > 1:
        out[int(crng.integers(0, len(out)))] = None
    return out


def with_colours(s, rgba):
    return types.SimpleNamespace(voxel_size=s.voxel_size, vps=s.vps, block_index=s.block_index, tsdf_distance=s.tsdf_distance,
                                 tsdf_weight=s.tsdf_weight, tsdf_rgba=rgba)


def main():
    from oracle import synth
    from profiles import fuzz_map_scene as S
    from tests import map_colour_ref as mc
    from tests import map_eval_ref as me
    from tests import map_query_ref as mq
    from tests import projected_map_ref as pm
    from voxgraph_amd import capi
    capi.load()
    ctx = capi.Context(0)
    n_seeds, first = int(os.environ.get("SEEDS", "100")), int(os.environ.get("FIRST", "0"))
    colour = os.environ.get("COLOUR", "0") == "1"
    deg = S.Degenerate()
    tot = dict(cases=0, blocks=0, points=0, voxels=0, coloured_blocks=0, blended=0)

    def fail(sc, product, msg):
        print("MISMATCH seed", sc.seed, "product", product, "\n ", msg, "\n ", S.describe(sc))
        return 1

    for seed in range(first, first + n_seeds):
        sc = S.draw(seed)
        vs, vps, rng = sc.voxel_size, sc.vps, sc.rng
        handles = [capi.Submap(ctx, i, vs, vps, s.block_index, s.tsdf_distance, s.tsdf_weight) for i, s in enumerate(sc.subs)]
        # 1. the merge, into an empty layer and into one with data and colours
        layer = capi.TsdfLayer(ctx, vs, vps)
        nb = layer.merge_submaps(handles, sc.poses)
        bi, d, w, rgba = layer.download()
        want = pm.merge_submaps({}, sc.subs, sc.poses)
        msg = S.compare_layers("merge into empty", layer_dict(bi, d, w), want)
        if msg or nb != len(want) or rgba.any():
            return fail(sc, "merge", msg or f"{nb} blocks reported, {len(want)} wanted, colours {bool(rgba.any())}")
        deg.count("merge", len(want) == 0)
        base_bi, base_d, base_w, base_rgba = sc.base
        full = capi.TsdfLayer(ctx, vs, vps)
        full.upload(base_bi, base_d, base_w, base_rgba)
        full.merge_submaps(handles, sc.poses)
        fbi, fd, fw, frgba = full.download()
        want_full = pm.merge_submaps(pm.layer_from_arrays(base_bi, base_d, base_w), sc.subs, sc.poses)
        msg = S.compare_layers("merge into a layer with data", layer_dict(fbi, fd, fw), want_full)
        if msg is None:
            slot = {tuple(int(v) for v in b): i for i, b in enumerate(fbi)}
            old = [slot[tuple(int(v) for v in b)] for b in base_bi]
            msg = S.compare("colours of the blocks that were there", frgba[old], base_rgba)
            new = np.setdiff1d(np.arange(len(fbi)), old)
            if msg is None and frgba[new].any():
                msg = "a newly allocated block has colours"
        if msg:
            return fail(sc, "merge", msg)
        full.destroy()
        tot["blocks"] += len(want) + len(want_full)
        tot["voxels"] += (len(want) + len(want_full)) * vps ** 3
        # 2. transformLayer of one submap
        k = seed % len(sc.subs)
        tl = capi.TsdfLayer(ctx, vs, vps)
        tl.transform_submap(handles[k], sc.transform_pose)
        tbi, td, tw, _ = tl.download()
        want_t = me.transform_layer(sc.subs[k], sc.transform_pose)
        msg = S.compare_layers("transform", layer_dict(tbi, td, tw), want_t)
        if msg:
            return fail(sc, "transform", msg + f" (submap {k}, pose {sc.transform_pose.tolist()})")
        deg.count("transform", len(want_t) == 0)
        tl.destroy()
        tot["blocks"] += len(want_t)
        tot["voxels"] += len(want_t) * vps ** 3
        # 6. the same with colours
        if colour:
            rgbas = draw_colours(seed, sc.subs, vps)
            csubs = [with_colours(s, c) for s, c in zip(sc.subs, rgbas)]
            for h, c in zip(handles, rgbas):
                if c is not None:
                    h.set_colors(c)
            for name, start in (("coloured merge into empty", None), ("coloured merge into a layer with data", sc.base)):
                cl = capi.TsdfLayer(ctx, vs, vps)
                if start is not None:
                    cl.upload(*start)
                cl.merge_submaps(handles, sc.poses)
                cbi, cd, cw, crgba = cl.download()
                want_c = mc.merge_submaps({} if start is None else mc.layer_from_arrays(*start), csubs, sc.poses)
                got_c = {tuple(int(v) for v in b): x for b, *x in zip(cbi, cd, cw, crgba)}
                msg = S.compare_layers(name, got_c, want_c)
                if msg:
                    return fail(sc, "coloured merge", msg + f" (colourless: {[i for i, c in enumerate(rgbas) if c is None]})")
                deg.count("coloured merge", len(want_c) == 0)
                tot["coloured_blocks"] += len(want_c)
                cl.destroy()
            kc = next((i for i in range(len(rgbas)) if rgbas[(k + i) % len(rgbas)] is not None), 0)
            kc = (k + kc) % len(rgbas)
            cl = capi.TsdfLayer(ctx, vs, vps)
            cl.transform_submap(handles[kc], sc.transform_pose)
            cbi, cd, cw, crgba = cl.download()
            want_c = mc.transform_submap(csubs[kc], sc.transform_pose)
            msg = S.compare_layers("coloured transform", {tuple(int(v) for v in b): x for b, *x in zip(cbi, cd, cw, crgba)}, want_c)
            if msg:
                return fail(sc, "coloured transform", msg + f" (submap {kc})")
            deg.count("coloured transform", len(want_c) == 0)
            tot["coloured_blocks"] += len(want_c)
            cl.destroy()
        for h in handles:
            h.destroy()
        if len(want) == 0:
            for _ in sc.queries:
                deg.count("query", True)
            for _ in sc.evals:
                deg.count("evaluation", True)
            layer.destroy()
            tot["cases"] += 1
            continue
        # 3. the projected map as a submap with an ESDF
        proj = capi.Submap.from_tsdf_layer(ctx, layer, 50)
        proj.generate_esdf()
        data = synth.SubmapData(vs, vps, proj.block_index(), *proj.download_layers(vps), np.zeros(4))
        # 4. queries
        for interp, grad, posed, lay in sc.queries:
            pose = sc.query_pose if posed else None
            p = S.query_points(rng, data, 4000, pose)
            got = proj.query(p, lay, interpolate=interp, gradient=grad, pose=pose, weight=lay == "tsdf")
            wd, wg, ww, wok = mq.query(data, p, lay, interpolate=interp, gradient=grad, pose=pose)
            msg = S.compare("valid", got.valid.view(np.uint8), wok.view(np.uint8)) or S.compare("distance", got.distance, wd)
            if msg is None and grad:
                msg = S.compare("gradient", got.gradient, wg)
            if msg is None and lay == "tsdf":
                msg = S.compare("weight", got.weight, ww)
            if msg:
                return fail(sc, "query", msg + f" ({lay} interpolate {interp} gradient {grad} pose {None if pose is None else pose.tolist()})")
            deg.count("query", wok.all() or not wok.any())
            tot["points"] += len(p)
        # 5. evaluation against a partly overlapping partner, as the test layer on even seeds
        partner = S.eval_partner(rng, data, vs, vps)
        ph = capi.Submap(ctx, 51, vs, vps, partner.block_index, partner.tsdf_distance, partner.tsdf_weight,
                         partner.esdf_distance, partner.esdf_observed)
        for lay, mode in sc.evals:
            (gd, gh), (td_, th) = ((partner, ph), (data, proj))[::1 if seed % 2 else -1]
            got, (ebi, ed, es) = capi.evaluate_layers_rmse(gh, th, lay, mode, error_layer=True)
            wdet, (wbi, wd, ws) = eval_reference(gd, td_, lay, mode, vps)
            msg = compare_details(got, wdet) or S.compare("error layer", (ebi, ed, es), (wbi, wd, ws))
            if msg:
                return fail(sc, "evaluation", msg + f" (layer {lay} mode {mode}, partner is {'gt' if seed % 2 else 'test'})")
            deg.count("evaluation", wdet["num_evaluated_voxels"] == 0)
            tot["voxels"] += wdet["num_overlapping_voxels"] + wdet["num_non_overlapping_voxels"]
        ph.destroy()
        proj.destroy()
        layer.destroy()
        tot["cases"] += 1
    ctx.close()
    over = deg.exceeded()
    print("degenerate cases per product:", {p: (deg.degenerate[p], n) for p, n in deg.cases.items()})
    if over:
        print("TOO MANY DEGENERATE CASES (more than one in five):", over)
        return 1
    print("no mismatch:", tot["cases"], "scenes,", tot["blocks"], "blocks,", tot["points"], "query points,", tot["voxels"],
          "voxels compared" + (f"; with colours {tot['coloured_blocks']} blocks (distance, weight, rgba)" if colour else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
