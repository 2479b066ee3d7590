"""The layer readers' fuzzer (profiles/fuzz_layer_readers.py) kept honest without a GPU, the counterpart of
tests/test_fuzz_map_cpu.py: over exactly the seed range tests/test_fuzz_gpu.py runs, the scene generator
(profiles/fuzz_reader_scene.py) and the numpy restatements alone must draw every class, meet every view status and both
localisation outcomes, stay under the cap on degenerate cases, really put the planted special voxels under the readers'
samples, and the comparator must report a flipped bit, a -0.0 / +0.0 swap and a changed count while it takes two NaNs of
different payload for equal.

The planted-voxel counts: every reader's sample goes through scan_registration_ref._neighbours.  The fixture wraps it and
looks the same positions up in two tag layers that hold, per voxel, which special was planted there.  A special DISTANCE
counts where the sample is valid (all 8 blocks exist, all 8 weights > 0: the value enters the trilinear form); a special
WEIGHT counts where all 8 blocks exist (the comparison w > 0 is what decides).  The restatements interpolate every point
of a scan and apply the stride and the range gate afterwards, so these counts include points that are no candidates."""
import copy
import importlib.util
import os

import numpy as np
import pytest

from profiles import fuzz_map_scene as S
from profiles import fuzz_reader_scene as RS
from tests import scan_registration_ref as SR
from tests import view_render_ref as V
from tests.test_fuzz_gpu import READERS

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuzzer(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "profiles", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FR = _fuzzer("fuzz_layer_readers")


def _address(a):
    return np.asarray(a).__array_interface__["data"][0]


class _Planted:
    """the wrapper of scan_registration_ref._neighbours: counts[reader][(kind, special index)] samples whose 8 neighbours
    include a voxel planted with that special; kind "distance" or "weight" """

    def __init__(self):
        self.tags, self.counts, self.reader, self.original = {}, {}, None, SR._neighbours

    def register(self, values, which_d, which_w):
        """the layer whose distance array is `values` (by its address: the restatements' layers are views of the scene's
        arrays) holds the planted indices which_d / which_w (int8 arrays of that shape, -1 for none; None for no array)"""
        self.tags[_address(values)] = (which_d, which_w)

    def __call__(self, L, p, FT):
        out = self.original(L, p, FT)
        tags = self.tags.get(_address(L.d)) if L.d.size else None
        if tags is not None and self.reader is not None:
            ok = out[0]
            for kind, which, specials in (("distance", tags[0], RS.DISTANCE_SPECIALS), ("weight", tags[1], RS.WEIGHT_SPECIALS)):
                if which is None:
                    continue
                tagged = copy.copy(L)
                tagged.d, tagged.w = which.astype(F).reshape(L.d.shape), np.ones(L.d.shape, F)
                present, code8, _ = self.original(tagged, p, FT)
                counted = ok if kind == "distance" else present
                tally = self.counts.setdefault(self.reader, {})
                for i in range(len(specials)):
                    hit = np.zeros(len(p), bool)
                    for code in code8:
                        hit |= code == i
                    tally[(kind, i)] = tally.get((kind, i), 0) + int((hit & counted).sum())
        return out


@pytest.fixture(scope="module")
def readers_run():
    """the restatements' side of fuzz_layer_readers over the suite's range"""
    deg, drawn, statuses = S.Degenerate(), {}, np.zeros(5, np.int64)
    outcomes = dict(usable=0, not_usable=0, none_eligible=0)
    planted = _Planted()
    seeds, first = READERS
    SR._neighbours = planted
    try:
        for seed in range(first, first + seeds):
            sc = RS.draw(seed)
            for k, v in sc.drawn.items():
                drawn.setdefault(k, set()).update(v)
            if sc.live_planted is not None:
                planted.register(sc.live[1], *sc.live_planted)
                tsdf = sc.map_cfg["layer"] == "tsdf"
                for sm, pl in zip(sc.subs, sc.planted):
                    planted.register(sm.tsdf_distance, pl["tsdf_distance"], pl["tsdf_weight"])
                    planted.register(sm.esdf_distance, pl["esdf_distance"], None)
                assert tsdf or all(pl["esdf_distance"] is not None for pl in sc.planted)
            planted.reader = "view"
            for _, view in FR.view_reference(sc):
                deg.count("view", FR.view_is_degenerate(view))
                statuses += np.bincount(view.status, minlength=5)
            planted.reader = "registration"
            ev, _ = FR.registration_reference(sc)
            deg.count("registration", ev[1] == 0)
            planted.reader = "localisation"
            lev, _, loc = FR.localisation_reference(sc)
            deg.count("evaluate_map", lev[1] == 0)
            deg.count("localize", loc[0] < 0)
            outcomes["none_eligible" if loc[0] < 0 else "usable" if loc[3]["usable"] else "not_usable"] += 1
            planted.reader = None
            planted.tags.clear()
    finally:
        SR._neighbours = planted.original
    return deg, drawn, statuses, outcomes, planted.counts


def test_the_same_seed_gives_the_same_scene():
    a, b = RS.draw(READERS[1] + 4), RS.draw(READERS[1] + 4)
    assert RS.describe(a) == RS.describe(b) and a.value_kind == "specials"
    assert S.compare("live", a.live + a.live_planted, b.live + b.live_planted) is None
    for x, y, px, py in zip(a.subs, b.subs, a.planted, b.planted):
        assert S.compare("submap", (x.block_index, x.tsdf_distance, x.tsdf_weight, x.esdf_distance, x.esdf_observed, *px.values()),
                         (y.block_index, y.tsdf_distance, y.tsdf_weight, y.esdf_distance, y.esdf_observed, *py.values())) is None
    assert S.compare("rest", (a.poses, a.listed_poses, a.T_sensor, a.T_view_submap, a.dirs, a.points, a.hyp, a.scored),
                     (b.poses, b.listed_poses, b.T_sensor, b.T_view_submap, b.dirs, b.points, b.hyp, b.scored)) is None
    assert a.listed == b.listed and RS.describe(RS.draw(READERS[1] + 5)) != RS.describe(a)


def test_fuzz_map_scenes_are_untouched_by_the_readers_draw():
    """the readers' scenes come from a stream of their own: drawing one between two draws of a map scene changes nothing"""
    a = S.draw(READERS[1])
    RS.draw(READERS[1])
    b = S.draw(READERS[1])
    assert S.describe(a) == S.describe(b)


def test_every_class_is_drawn_in_the_suites_range(readers_run):
    drawn = readers_run[1]
    assert drawn["value_kind"] == set(RS.VALUE_KINDS) and "specials" in drawn["value_kind"]
    assert drawn["vps"] == {8, 16}
    assert drawn["voxel_size"] == {float(F(v)) for v in S.VOXEL_SIZES}
    assert drawn["far_box"] == {False, True}
    assert drawn["pose_kind"] == set(S.POSE_KINDS)
    assert drawn["shape"] == set(S.SHAPE_KINDS)
    assert drawn["n_submaps"] == set(RS.N_SUBMAPS)
    assert drawn["empty_submap"] == {False, True} and drawn["duplicate"] == {False, True}
    assert drawn["layer"] == set(RS.LAYERS) and drawn["huber_finite"] == {False, True}
    assert drawn["point_stride"] == set(RS.STRIDES) and drawn["score_point_stride"] == set(RS.STRIDES)
    assert drawn["n_points"] == set(RS.POINT_SIZES) and drawn["n_poses"] == set(RS.N_POSES)
    assert drawn["rays"] == {("image", w, h) for w, h in RS.IMAGES} | {("rays", n) for n in RS.RAY_SIZES}
    assert drawn["max_iterations"] == set(RS.MAX_ITERATIONS) and max(RS.MAX_ITERATIONS) <= 8


def test_the_far_boxes_reach_two_to_the_twenty():
    """over a longer range than the suite's the offsets come within 2^13 blocks of 2^20 -- and never past the 21 bits per
    axis of the restatement's block key, with 4000 blocks to spare for the samples around the box"""
    largest = max(int(np.abs(RS.draw(seed).offset).max()) for seed in range(1, 400, 4))
    assert (1 << 20) - (1 << 13) < largest <= RS.FAR_LIMIT


def test_every_view_status_and_both_localisation_outcomes_occur(readers_run):
    _, _, statuses, outcomes, _ = readers_run
    assert (statuses > 0).all(), dict(zip(("MISS", "HIT", "INSIDE", "BAD", "HIT_UNSAMPLED"), statuses.tolist()))
    assert (V.MISS, V.HIT, V.INSIDE, V.BAD, V.HIT_UNSAMPLED) == (0, 1, 2, 3, 4)
    assert outcomes["usable"] > 0 and outcomes["none_eligible"] > 0, outcomes


def test_at_most_one_case_in_five_is_degenerate(readers_run):
    deg = readers_run[0]
    assert set(deg.cases) == set(FR.PRODUCTS)
    assert not deg.exceeded(), (deg.exceeded(), deg.degenerate)
    assert deg.cases["view"] == 2 * READERS[0] and all(deg.cases[p] == READERS[0] for p in FR.PRODUCTS[1:])


def test_the_specials_reach_the_arithmetic(readers_run):
    counts = readers_run[4]
    assert set(counts) == {"view", "registration", "localisation"}
    for reader, tally in counts.items():
        for i, value in enumerate(RS.DISTANCE_SPECIALS):
            assert tally.get(("distance", i), 0) > 0, (reader, "distance", float(value), tally)
        for i, value in enumerate(RS.WEIGHT_SPECIALS):
            assert tally.get(("weight", i), 0) > 0, (reader, "weight", float(value), tally)


def test_the_specials_are_the_issues_values_and_are_planted_independently():
    d, w = RS.DISTANCE_SPECIALS, RS.WEIGHT_SPECIALS
    assert d.dtype == F and w.dtype == F and len(d) == 8 and len(w) == 7
    assert np.isnan(d[0]) and d[1] == np.inf and d[2] == -np.inf and d[3] == 0 and np.signbit(d[3]) and d[4] == 0 and not np.signbit(d[4])
    assert 0 < d[5] < np.finfo(F).tiny and -np.finfo(F).tiny < d[6] < 0 and d[7] == F(3e38)          # denormals: below the smallest normal
    assert np.isnan(w[0]) and w[1] == np.inf and w[2] == 0 and np.signbit(w[2]) and w[3] == 0 and not np.signbit(w[3]) and w[4] == -1
    assert 0 < w[6] < w[5] < np.finfo(F).tiny and w[6].view(np.uint32) == 1                       # 1e-45: the smallest denormal
    sc = RS.draw(READERS[1] + 4)
    which_d, which_w = sc.live_planted
    pd, pw = which_d >= 0, which_w >= 0
    assert 0.015 < pd.mean() < 0.025 and 0.015 < pw.mean() < 0.025
    with np.errstate(invalid="ignore"):
        assert (pd & (sc.live[2] > 0)).sum() > 0.5 * pd.sum()                       # a special distance under a valid weight
    for i in range(len(d)):
        assert np.array_equal(sc.live[1][which_d == i].view(np.uint32), np.full(int((which_d == i).sum()), d[i].view(np.uint32)))


def test_the_comparator_reports_a_flipped_bit_a_zero_sign_and_a_changed_count():
    sc = RS.draw(READERS[1] + 3)
    (name, view), _ = FR.view_reference(sc)
    got = lambda: V.View(**{k: (v.copy() if isinstance(v, np.ndarray) else dict(v)) for k, v in vars(view).items()})
    assert FR.compare_view(name, got(), dict(view.counts), view) is None
    for field in FR.VIEW_ARRAYS:
        g = got()
        flat = getattr(g, field).reshape(-1).view(np.uint8)
        flat[len(flat) // 2] ^= 1                                                  # one bit of one array
        msg = FR.compare_view(name, g, dict(view.counts), view)
        assert msg and field in msg and "1 of" in msg, msg
    msg = FR.compare_view(name, got(), dict(view.counts, n_samples=view.counts["n_samples"] + 1), view)
    assert msg and "counts" in msg
    # -0.0 is not +0.0, with the NaN rule and without it
    a, b = np.zeros(4, F), np.zeros(4, F)
    b[2] = F(-0.0)
    assert a[2] == b[2] and "1 of 4" in S.compare("zeros", a, b) and "1 of 4" in S.compare("zeros", a, b, nan_equal=True)
    # two NaNs of different sign and payload: equal under the rule, different by default; a NaN is no number
    x = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x3f800000], np.uint32).view(F)
    y = np.array([0xffc00000, 0x7fc00001, 0x7fc00000, 0x3f800000], np.uint32).view(F)
    assert S.compare("nans", x, y, nan_equal=True) is None and "3 of 4" in S.compare("nans", x, y)
    assert S.compare("nans", (x, None), (y, None), nan_equal=True) is None
    y[3] = np.nan
    assert "1 of 4" in S.compare("nans", x, y, nan_equal=True)
    d = np.array([np.nan, 1.0]), np.array([-np.nan, 1.0])
    assert S.compare("f64", d[0], d[1], nan_equal=True) is None
    assert "1 of 2" in S.compare("f64", d[0], np.array([np.nan, np.nextafter(1.0, 2)]), nan_equal=True)
    # the sums and counts of an evaluation, the scores, a refinement
    out = (np.arange(15.0), 3, 5)
    assert FR.compare_sums("e", out, (out[0].copy(), 3, 5)) is None
    assert "counts" in FR.compare_sums("e", out, (out[0], 3, 6))
    assert "sums" in FR.compare_sums("e", out, (np.nextafter(out[0], 99), 3, 5))
    scores = (np.array([0.5, 0.25]), np.array([3, 4]), np.array([2, 2]), np.array([9, 9]))
    assert FR.compare_scores("s", scores, tuple(x.copy() for x in scores)) is None
    assert "n_points_valid" in FR.compare_scores("s", scores, (scores[0], scores[1], np.array([2, 3]), scores[3]))
    assert "cost" in FR.compare_scores("s", scores, (np.array([0.5, -0.25]), *scores[1:]))
    summary = dict.fromkeys(FR.SUMMARY_INT, 1) | dict.fromkeys(FR.SUMMARY_F64, 0.5) | dict(termination="max_iterations")
    rec = dict.fromkeys(FR.HISTORY_F64, 0.25) | dict.fromkeys(FR.HISTORY_INT, 0)
    got_r, want_r = (np.ones(7, F), True, np.zeros(4), summary), (np.ones(7, F), np.zeros(4), summary, [rec])
    assert FR.compare_refinement("r", got_r, [dict(rec)], want_r) is None
    assert "history[0]" in FR.compare_refinement("r", got_r, [rec | dict(accepted=1)], want_r)
    assert "history" in FR.compare_refinement("r", got_r, [rec | dict(radius=np.nextafter(0.25, 1))], want_r)
    assert "history of 0" in FR.compare_refinement("r", got_r, [], want_r)
    assert "num_iterations" in FR.compare_refinement("r", (got_r[0], True, got_r[2], summary | dict(num_iterations=2)), [rec], want_r)
    assert "delta" in FR.compare_refinement("r", (got_r[0], True, np.array([0, 0, 0, -0.0]), summary), [rec], want_r)
