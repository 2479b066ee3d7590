#!/usr/bin/env python3
"""Differential fuzzing of the three readers of a layer -- view rendering (vgx_view.hip), scan-to-map registration
(vgx_scan_reg.hip) and scan localisation (vgx_scan_localize.hip) -- against their numpy restatements
(tests/view_render_ref.py, tests/scan_registration_ref.py, tests/scan_localization_ref.py) on the scenes of
profiles/fuzz_reader_scene.py: block boxes up to 2^20 blocks from the origin, dyadic and odd voxel sizes, grid-aligned poses,
one-block layers and slabs, planted validity thresholds, and voxels that hold NaN, +-inf, -0.0, denormals, 3e38 and negative
weights.  Per seed:
  1. views: vgx_tsdf_layer_render_view on the uploaded live layer and vgx_submap_render_view on one finished submap, every
     flag, against view_render_ref.render -- range, status, points, gradient, weight, rgba, n_samples and the counts; the
     organised and the unorganised launch of the same rays must give the same bytes;
  2. scan-to-map registration on the live layer: evaluate at a drawn correction (15 sums, both counts) and refine with at
     most 8 iterations (T_refined, delta, the summary, the whole history);
  3. localisation on the listed submaps (one of them of zero blocks or listed twice on some seeds; 1, 2, 3 or 5 of them),
     layer and Huber scale as drawn: evaluate_map, score_poses (every pose up to 7, a drawn 8 of 65; each equal to half the
     cost of evaluate_map at that pose on a handle whose point_stride is the score stride), and localize (best index,
     refined pose, summary, history).
Everything is compared by its bits, with one exception: a NaN equals a NaN whatever its sign and payload (a kernel and x86
numpy give different default NaNs for inf - inf); -0.0 is not +0.0.  A view without a HIT, an evaluation without a term and
a localisation without an eligible hypothesis count as degenerate; more than one in five per product fails.
    SEEDS=200 FIRST=1000 python profiles/fuzz_layer_readers.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
VIEW_ARRAYS = ("range", "status", "points", "gradient", "weight", "rgba", "n_samples")
SUMMARY_INT = ("usable", "termination", "num_iterations", "num_successful_steps", "num_evaluations", "num_factorization_failures",
               "n_candidates", "n_valid_first", "n_valid_last")
SUMMARY_F64 = ("initial_cost", "final_cost")
HISTORY_F64 = ("cost", "trial_cost", "gain_ratio", "radius", "step_norm")
HISTORY_INT = ("accepted", "factorization_failed")
PRODUCTS = ("view", "registration", "evaluate_map", "localize")


# ---------------------------------------------------------------------------
# the restatements' side: what tests/test_fuzz_readers_cpu.py runs alone
# ---------------------------------------------------------------------------
def view_layers(sc):
    """(the live layer, the viewed submap) as view_render_ref layers"""
    from tests import view_render_ref as V
    sm = sc.subs[sc.view_submap]
    return (V.layer_of(sc.voxel_size, sc.vps, *sc.live),
            V.layer_of(sc.voxel_size, sc.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight, sc.submap_rgba))


def view_reference(sc):
    """-> [(name, view_render_ref.View)]: the live layer's view, the submap's"""
    from tests import view_render_ref as V
    live, sub = view_layers(sc)
    cfg = V.config(**sc.view_cfg)
    return [("live layer", V.render(live, sc.T_sensor, sc.dirs, cfg)), ("submap", V.render(sub, sc.T_view_submap, sc.dirs, cfg))]


def registration_layer(sc):
    from tests import scan_registration_ref as SR
    return SR.layer_of(sc.voxel_size, sc.vps, *sc.live[:3])


def registration_reference(sc):
    """-> (evaluate's (out, n_valid, n_candidates), refine's (T, delta, summary, history))"""
    from tests import scan_registration_ref as SR
    L, cfg = registration_layer(sc), SR.config(**sc.reg_cfg)
    return (SR.evaluate(L, sc.points, sc.T_sensor, sc.delta, cfg),
            SR.refine(L, sc.points, sc.T_sensor, cfg, max_num_iterations=sc.max_iterations))


def localisation_map(sc):
    from profiles import fuzz_reader_scene as RS
    from tests import scan_localization_ref as R
    return R.Map(RS.listed_submaps(sc), sc.listed_poses, sc.map_cfg["layer"])


def localisation_reference(sc):
    """-> (evaluate_map's result, score_poses' over sc.scored, localize's (best, T, delta, summary, history))"""
    from tests import scan_localization_ref as R
    from tests import scan_registration_ref as SR
    M, cfg, mcfg = localisation_map(sc), SR.config(**sc.loc_cfg), R.map_config(**sc.map_cfg)
    ev = R.evaluate_map(M, sc.points, sc.T_sensor, sc.loc_delta, cfg, mcfg)
    if len(sc.scored) == len(sc.hyp):
        scores = R.score_poses(M, sc.points, sc.hyp, cfg, mcfg)
        picked = scores
    else:
        scores = None
        picked = R.score_poses(M, sc.points, sc.hyp[sc.scored], cfg, mcfg)
    loc = R.localize(M, sc.points, sc.hyp, cfg, mcfg, scores=scores, max_num_iterations=sc.max_iterations)
    return ev, picked, loc


# ---------------------------------------------------------------------------
# comparisons: by bits, a NaN equal to a NaN
# ---------------------------------------------------------------------------
def compare_view(name, got, counts, want):
    """got: capi.ViewImage, counts: View.stats(); want: view_render_ref.View"""
    from profiles import fuzz_map_scene as S
    if counts != want.counts:
        return f"{name}: counts {counts}, want {want.counts}"
    for field in VIEW_ARRAYS:
        msg = S.compare(f"{name} {field}", getattr(got, field), getattr(want, field), nan_equal=True)
        if msg:
            return msg
    return None


def compare_sums(name, got, want):
    """(out [15] f64, counts...) of an evaluation"""
    from profiles import fuzz_map_scene as S
    if tuple(int(v) for v in got[1:]) != tuple(int(v) for v in want[1:]):
        return f"{name}: counts {tuple(got[1:])}, want {tuple(want[1:])}"
    return S.compare(f"{name} sums", np.asarray(got[0], np.float64), np.asarray(want[0], np.float64), nan_equal=True)


def compare_refinement(name, got, history, want):
    """got: (T, usable, delta, summary) of capi's refine / refine_map, history: reg.history(); want: the restatement's
    (T, delta, summary, history)"""
    from profiles import fuzz_map_scene as S
    T, usable, delta, summary = got
    wT, wdelta, wsummary, whistory = want
    for key in SUMMARY_INT:
        if summary[key] != wsummary[key]:
            return f"{name}: summary {key} {summary[key]}, want {wsummary[key]}"
    if usable != bool(wsummary["usable"]):
        return f"{name}: usable {usable}"
    if len(history) != len(whistory):
        return f"{name}: history of {len(history)}, want {len(whistory)}"
    for k, (h, wh) in enumerate(zip(history, whistory)):
        if any(h[key] != wh[key] for key in HISTORY_INT):
            return f"{name}: history[{k}] {h}, want {wh}"
    return (S.compare(f"{name} T_refined", np.asarray(T, F), np.asarray(wT, F), nan_equal=True)
            or S.compare(f"{name} delta", np.asarray(delta, np.float64), np.asarray(wdelta, np.float64), nan_equal=True)
            or S.compare(f"{name} summary costs", np.array([summary[k] for k in SUMMARY_F64], np.float64),
                         np.array([wsummary[k] for k in SUMMARY_F64], np.float64), nan_equal=True)
            or S.compare(f"{name} history", np.array([[h[k] for k in HISTORY_F64] for h in history], np.float64).reshape(-1, 5),
                         np.array([[h[k] for k in HISTORY_F64] for h in whistory], np.float64).reshape(-1, 5), nan_equal=True))


def compare_scores(name, got, want):
    """(cost [m] f64, n_terms, n_points_valid, n_candidates)"""
    from profiles import fuzz_map_scene as S
    for g, w, what in zip(got[1:], want[1:], ("n_terms", "n_points_valid", "n_candidates")):
        if not np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)):
            return f"{name}: {what} {np.asarray(g).tolist()}, want {np.asarray(w).tolist()}"
    return S.compare(f"{name} cost", np.asarray(got[0], np.float64), np.asarray(want[0], np.float64), nan_equal=True)


def view_is_degenerate(view):
    return view.counts["n_hit"] == 0


# ---------------------------------------------------------------------------
def main():
    from profiles import fuzz_map_scene as S
    from profiles import fuzz_reader_scene as RS
    from voxgraph_amd import capi
    capi.load()
    ctx = capi.Context(0)
    n_seeds, first = int(os.environ.get("SEEDS", "100")), int(os.environ.get("FIRST", "0"))
    deg = S.Degenerate()
    tot = dict(cases=0, rays=0, points=0, hypotheses=0)

    def fail(sc, product, msg):
        print("MISMATCH seed", sc.seed, "product", product, "\n ", msg, "\n ", RS.describe(sc))
        return 1

    for seed in range(first, first + n_seeds):
        sc = RS.draw(seed)
        vs, vps = sc.voxel_size, sc.vps
        live = capi.TsdfLayer(ctx, vs, vps)
        live.upload(*sc.live)
        handles = [capi.Submap(ctx, k, vs, vps, s.block_index, s.tsdf_distance, s.tsdf_weight, s.esdf_distance, s.esdf_observed)
                   for k, s in enumerate(sc.subs)]
        e = RS.empty_submap(sc)
        empty = capi.Submap(ctx, len(handles), vs, vps, e.block_index, e.tsdf_distance, e.tsdf_weight, e.esdf_distance, e.esdf_observed)
        if sc.submap_rgba is not None:
            handles[sc.view_submap].set_colors(sc.submap_rgba)

        # 1. views: the image's launch and the unorganised one
        width = sc.image[0]
        tiled = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, image_width=width, **sc.view_cfg))
        linear = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **sc.view_cfg))
        sources = ((live, sc.T_sensor), (handles[sc.view_submap], sc.T_view_submap))
        for (source, T), (name, want) in zip(sources, view_reference(sc)):
            a = source.render_view(tiled, T, sc.dirs).download()
            msg = compare_view(f"{name}, image_width {width}", a, tiled.stats(), want)
            b = source.render_view(linear, T, sc.dirs).download()
            msg = msg or compare_view(f"{name}, unorganised", b, linear.stats(), want)
            msg = msg or S.compare(f"{name}: the two launches", tuple(b), tuple(a))          # the same bytes, NaNs included
            if msg:
                return fail(sc, "view", msg)
            deg.count("view", view_is_degenerate(want))
            tot["rays"] += 2 * len(sc.dirs)
        tiled.destroy()
        linear.destroy()

        # 2. scan-to-map registration on the live layer
        want_ev, want_rf = registration_reference(sc)
        reg = capi.ScanRegistration(ctx, capi.scan_registration_config(**sc.reg_cfg))
        reg.set_points(sc.points)
        msg = compare_sums("evaluate", reg.evaluate(live, sc.T_sensor, sc.delta), want_ev)
        if msg is None:
            got = reg.refine(live, sc.T_sensor, max_num_iterations=sc.max_iterations)
            msg = compare_refinement("refine", got, reg.history(), want_rf)
        if msg:
            return fail(sc, "registration", msg)
        deg.count("registration", want_ev[1] == 0)
        reg.destroy()
        tot["points"] += len(sc.points) * (1 + want_rf[2]["num_evaluations"])

        # 3. localisation on the listed submaps
        want_ev, want_scores, want_loc = localisation_reference(sc)
        listed = [handles[k] if k >= 0 else empty for k in sc.listed]
        loc = capi.ScanRegistration(ctx, capi.scan_registration_config(**sc.loc_cfg))
        loc.set_map(listed, sc.listed_poses, capi.scan_map_config(**sc.map_cfg))
        loc.set_points(sc.points)
        msg = compare_sums("evaluate_map", loc.evaluate_map(sc.T_sensor, sc.loc_delta), want_ev)
        if msg is None:
            scores = loc.score_poses(sc.hyp)
            msg = compare_scores("score_poses", tuple(x[sc.scored] for x in scores), want_scores)
        if msg is None:
            # a score is half the cost of the evaluation at that pose, where the evaluation's stride is the score's
            same = capi.ScanRegistration(ctx, capi.scan_registration_config(**dict(sc.loc_cfg, point_stride=sc.map_cfg["score_point_stride"])))
            same.set_map(listed, sc.listed_poses, capi.scan_map_config(**sc.map_cfg))
            same.set_points(sc.points)
            for m in sc.scored:
                out, nt, nv, nc = same.evaluate_map(sc.hyp[m])
                msg = msg or compare_scores(f"score_poses[{m}] against evaluate_map", tuple(np.array([x[m]]) for x in scores),
                                            (np.array([0.5 * out[0]]), [nt], [nv], [nc]))
            same.destroy()
        if msg is None:
            best, T, usable, delta, summary = loc.localize(sc.hyp, max_num_iterations=sc.max_iterations)
            if best != want_loc[0]:
                msg = f"localize: best {best}, want {want_loc[0]}"
            else:
                msg = compare_refinement("localize", (T, usable, delta, summary), loc.history(), want_loc[1:])
        if msg:
            return fail(sc, "localisation", msg)
        deg.count("evaluate_map", want_ev[1] == 0)
        deg.count("localize", want_loc[0] < 0)
        loc.destroy()
        tot["hypotheses"] += len(sc.hyp)
        tot["points"] += len(sc.points) * (1 + len(sc.scored) + want_loc[3]["num_evaluations"]) + len(sc.points) * len(sc.hyp)
        for x in handles + [empty, live]:
            x.destroy()
        tot["cases"] += 1
    ctx.close()
    over = deg.exceeded()
    print("degenerate cases per product:", {p: (deg.degenerate[p], n) for p, n in deg.cases.items()})
    if over:
        print("TOO MANY DEGENERATE CASES (more than one in five):", over)
        return 1
    print("no mismatch:", tot["cases"], "scenes,", tot["rays"], "rays,", tot["points"], "point evaluations,", tot["hypotheses"], "hypotheses")
    return 0


if __name__ == "__main__":
    sys.exit(main())
