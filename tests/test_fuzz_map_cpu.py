"""The map-product fuzzers (profiles/fuzz_map_layers.py, profiles/fuzz_map_meshes.py) kept honest without a GPU: over
exactly the seed ranges tests/test_fuzz_gpu.py runs, the scene generator (profiles/fuzz_map_scene.py) and the numpy
restatements alone must draw every class, stay under the cap on degenerate cases, really produce the ties the fuzzers
are there for, and the fuzzers' compare function must report a flipped bit and a dropped triangle.

Where the GPU fuzzer reads the device's ESDF of the projected map (queries and evaluation), this file has none: it
takes the merged TSDF layer as the ESDF too (distance = the TSDF distance, observed = weight > 0).  The block sets, the
points and the flags are those of the GPU run; the GPU fuzzers count the degenerate cases of their own data again."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import synth
from profiles import fuzz_map_scene as S
from tests import map_eval_ref as me
from tests import map_query_ref as mq
from tests import mesh_ref as mr
from tests import projected_map_ref as pm
from tests import separated_mesh_ref as sr
from tests.test_fuzz_gpu import MAP_LAYERS, MAP_MESHES

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuzzer(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "profiles", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FL, FM = _fuzzer("fuzz_map_layers"), _fuzzer("fuzz_map_meshes")
_merged = {}


def _merge(sc):
    if sc.seed not in _merged:
        _merged[sc.seed] = pm.merge_submaps({}, sc.subs, sc.poses)
    return _merged[sc.seed]


def _tally(total, drawn):
    for k, v in drawn.items():
        total.setdefault(k, set()).update(v)


def _on_grid(sc, blocks):
    """coordinates of the merge's sample points T_S_L * c whose p * voxel_size_inv is an exact integer: on a voxel face,
    the decision boundary of floorf(x * inv + 1e-6f), which is taken per axis"""
    if not len(blocks):
        return 0
    c = pm.block_centres(np.array(sorted(blocks)), sc.vps, F(sc.voxel_size))
    inv = F(F(1) / F(sc.voxel_size))
    n = 0
    for T in sc.poses:
        qi, ti = pm.inverse(T)
        x = (pm.transform(qi, ti, c) * inv).astype(F)
        n += int((x == np.rint(x)).sum())
    return n


@pytest.fixture(scope="module")
def layers_run():
    """the restatements' side of fuzz_map_layers over the suite's range"""
    deg, drawn, on_grid = S.Degenerate(), {}, 0
    seeds, first = MAP_LAYERS
    for seed in range(first, first + seeds):
        sc = S.draw(seed)
        _tally(drawn, sc.drawn)
        vs, vps = sc.voxel_size, sc.vps
        want = _merge(sc)
        deg.count("merge", len(want) == 0)
        on_grid += _on_grid(sc, list(want))
        deg.count("transform", len(me.transform_layer(sc.subs[seed % len(sc.subs)], sc.transform_pose)) == 0)
        if not want:
            for _ in sc.queries:
                deg.count("query", True)
            for _ in sc.evals:
                deg.count("evaluation", True)
            continue
        bi = np.array(list(want), np.int32)
        td = np.stack([want[k][0] for k in want])
        tw = np.stack([want[k][1] for k in want])
        data = synth.SubmapData(vs, vps, bi, td, tw, td, (tw > 0).astype(np.uint8), np.zeros(4))
        for interp, grad, posed, lay in sc.queries:
            pose = sc.query_pose if posed else None
            ok = mq.query(data, S.query_points(sc.rng, data, 4000, pose), lay, interpolate=interp, gradient=grad, pose=pose)[3]
            deg.count("query", ok.all() or not ok.any())
        partner = S.eval_partner(sc.rng, data, vs, vps)
        for lay, mode in sc.evals:
            gt, test = (partner, data) if seed % 2 else (data, partner)
            deg.count("evaluation", FL.eval_reference(gt, test, lay, mode, vps)[0]["num_evaluated_voxels"] == 0)
    return deg, drawn, on_grid


@pytest.fixture(scope="module")
def meshes_run():
    """the restatements' side of fuzz_map_meshes over the suite's range"""
    deg, drawn = S.Degenerate(), {}
    ties = dict(half=0, zero_pos=0, zero_neg=0, largest_key=0)
    seeds, first = MAP_MESHES
    for seed in range(first, first + seeds):
        sc = S.draw(seed)
        _tally(drawn, sc.drawn)
        vs, vps, mw = sc.voxel_size, sc.vps, sc.min_weight
        layer = _merge(sc)
        bi = np.array(list(layer), np.int32).reshape(-1, 3)
        d = np.stack([layer[k][0] for k in layer]) if layer else np.zeros((0, vps ** 3), F)
        w = np.stack([layer[k][1] for k in layer]) if layer else np.zeros((0, vps ** 3), F)
        k, order = seed % len(sc.subs), sc.sep_order
        sub = [(s.block_index, s.tsdf_distance, s.tsdf_weight) for s in sc.subs]
        meshes = [("combined mesh", mr.generate_mesh(bi, d, w, vps, vs, mw)[:4]),
                  ("submap mesh", mr.generate_mesh(*sub[k], vps, vs, mw)[:4]),
                  ("separated mesh", sr.separated_mesh([sub[i] for i in order], sc.poses[order], sc.colors[order], vps, vs, mw))]
        for m, (name, want) in enumerate(meshes):
            deg.count(name, len(want[2]) == 0)
            soup = (want[2], want[3], want[4] if len(want) > 4 else None)
            v = want[2].reshape(-1, 3)
            ties["zero_pos"] += int(((v == 0) & ~np.signbit(v)).sum())
            ties["zero_neg"] += int(((v == 0) & np.signbit(v)).sum())
            for kind, thr in sc.thresholds[2 * m:2 * m + 2]:
                wc = FM.connect_reference(soup, thr)
                deg.count("connected " + name, FM.weld_is_degenerate(wc))
                ties["largest_key"] = max(ties["largest_key"], FM.largest_weld(wc))
                if wc is not None and len(v):
                    x = np.abs(v.astype(np.float64) * (np.float64(1.0) / np.float64(thr)))
                    ties["half"] += int((x - np.floor(x) == 0.5).sum())
    return deg, drawn, ties


def test_the_same_seed_gives_the_same_scene():
    a, b = S.draw(MAP_LAYERS[1] + 3), S.draw(MAP_LAYERS[1] + 3)
    assert S.describe(a) == S.describe(b) and len(a.subs) == len(b.subs)
    for x, y in zip(a.subs, b.subs):
        assert S.compare("submap", (x.block_index, x.tsdf_distance, x.tsdf_weight), (y.block_index, y.tsdf_distance, y.tsdf_weight)) is None
    assert S.compare("rest", (a.poses, a.colors, a.query_pose, a.transform_pose) + a.base,
                     (b.poses, b.colors, b.query_pose, b.transform_pose) + b.base) is None
    assert np.array_equal(S.query_points(a.rng, a.subs[0], 100), S.query_points(b.rng, b.subs[0], 100))
    assert S.describe(S.draw(MAP_LAYERS[1] + 4)) != S.describe(a)


def _assert_every_class(drawn):
    assert drawn["voxel_size"] == {float(F(v)) for v in S.VOXEL_SIZES}
    assert drawn["vps"] == {8, 16}
    assert drawn["min_weight"] == set(S.MIN_WEIGHTS)
    assert drawn["pose_kind"] == set(S.POSE_KINDS)
    assert drawn["value_kind"] == set(S.VALUE_KINDS)
    assert drawn["shape"] == set(S.SHAPE_KINDS)
    assert drawn["threshold_kind"] == set(S.THRESHOLD_KINDS)
    assert drawn["eval"] == set(S.EVAL_COMBOS) and len(S.EVAL_COMBOS) == 8
    assert drawn["query"] == set(S.QUERY_COMBOS) and len(S.QUERY_COMBOS) == 8       # 4 flag combinations, posed and not
    assert drawn["query_layer"] == {"esdf", "tsdf"}
    assert drawn["duplicate_entry"] == {False, True}
    assert drawn["offset_sign"] == {-1, 0, 1}
    assert {1, 2}.issubset({min(n, 2) for n in drawn["n_submaps"]})                   # a single submap, and several


def test_every_class_is_drawn_in_the_suites_ranges(layers_run, meshes_run):
    _assert_every_class(layers_run[1])
    _assert_every_class(meshes_run[1])


def test_at_most_one_case_in_five_is_degenerate(layers_run, meshes_run):
    for deg, products in ((layers_run[0], {"merge", "transform", "query", "evaluation"}),
                          (meshes_run[0], {"combined mesh", "submap mesh", "separated mesh", "connected combined mesh",
                                           "connected submap mesh", "connected separated mesh"})):
        assert set(deg.cases) == products                                             # no product, and no seed, left out
        assert not deg.exceeded(), (deg.exceeded(), deg.degenerate)
    assert layers_run[0].cases["merge"] == MAP_LAYERS[0] and meshes_run[0].cases["separated mesh"] == MAP_MESHES[0]


def test_the_ties_really_occur(layers_run, meshes_run):
    """Soup vertices on exact half cells of the weld grid, sample points on exact voxel-grid integers, one key that
    takes more than 1000 soup vertices, and vertex coordinates that are exactly zero.
    Both signs of zero cannot be drawn: no mesh the library makes holds a -0.0 coordinate.  A voxel centre
    origin + (idx + 0.5) * voxel_size is never zero; a vertex pa + t * (pb - pa) or 0.5 * (pa + pb) is zero only by
    cancellation, which gives +0.0 in round-to-nearest; the separated mesh's (v + w * uv) + (u x uv) and its + t are
    sums with that +0.0 or with non-zero terms, and a sum is -0.0 only when both its terms are.  So the soups are
    checked to hold +0.0 and no -0.0 (a -0.0 would falsify this reasoning and is worth knowing), and the -0.0 key rule
    stays with tests/test_connected_mesh_cpu.py."""
    ties = meshes_run[2]
    assert ties["half"] > 0, ties
    assert ties["largest_key"] > 1000, ties
    assert ties["zero_pos"] > 0 and ties["zero_neg"] == 0, ties
    assert layers_run[2] > 0


def test_the_comparator_reports_a_flipped_bit_and_a_dropped_triangle():
    sc = S.draw(MAP_MESHES[1])
    s = sc.subs[0]
    want = mr.generate_mesh(s.block_index, s.tsdf_distance, s.tsdf_weight, sc.vps, sc.voxel_size, sc.min_weight)[:4]
    assert len(want[2]) > 10
    assert S.compare("mesh", tuple(a.copy() for a in want), want) is None
    for i in range(4):
        got = [a.copy() for a in want]
        flat = got[i].reshape(-1).view(np.uint8)
        flat[len(flat) // 2] ^= 1                                                    # one bit of one array
        msg = S.compare("mesh", tuple(got), want)
        assert msg and f"mesh[{i}]" in msg and "1 of" in msg, msg
    got = (want[0], want[1], want[2][:-1], want[3][:-1])
    msg = S.compare("mesh", got, want)
    assert msg and "shape" in msg and "mesh[2]" in msg, msg
    assert "None" in S.compare("colours", None, np.zeros(3, np.uint8))
    a = {(0, 0, 0): (np.zeros(8, F), np.ones(8, F))}
    b = {(0, 0, 0): (np.zeros(8, F), np.ones(8, F))}
    assert S.compare_layers("layer", a, b) is None
    b[(0, 0, 0)][0][3] = F(-0.0)                                                     # equal as values, not as bits
    assert "block (0, 0, 0)" in S.compare_layers("layer", a, b)
    assert "block sets differ" in S.compare_layers("layer", a, {})
    det = dict.fromkeys(FL.DETAILS_INT, 1) | dict.fromkeys(FL.DETAILS_F64, 0.5)
    assert FL.compare_details(det, dict(det)) is None
    assert "total_squared_error" in FL.compare_details(det, det | {"total_squared_error": np.nextafter(0.5, 1)})
    assert "num_ignored_voxels" in FL.compare_details(det, det | {"num_ignored_voxels": 2})
