"""The registration batch's sequence fuzzer (profiles/fuzz_reg_sequences.py) kept honest without a GPU: over exactly the
seed range tests/test_fuzz_gpu.py runs, the generator (profiles/fuzz_reg_sequence_scene.py) must draw every op kind, every
pose class as the first evaluation of each pass, every arm at least twice, every refused-call kind in a sampling and in
an all-points seed, the planted point counts and a set of fewer than 64 points; no seed may need more than one re-draw;
every call it lists as refused must be one by the header's rules and every assembly / fetch it lists as valid must have
something defined to read (the sequences are replayed through a model written here, not the generator's).

The "shared" arm's launch-order decision is restated from its documented inputs (make_xcd_order: chunk bounding spheres
against the reading grid's block box at the poses of each pass's first evaluation): at least 16 tiles in either pass,
shareable >= 0.3 of the loaded points, loaded >= 0.75 of all points; the far-first seeds load nothing at their first poses.

Where oracle/_ref is built, every sampling seed's sequence also runs through the reference's own compiled
RegistrationCostFunction -- one Evaluate per constraint per evaluation in list order, one Evaluate for a drop-in, nothing
for a count, a refused call, a fetch, an assembly -- and the model's rows must equal its rows."""
import numpy as np
import pytest

from oracle import ref_reg
from profiles import fuzz_reg_sequence_scene as SS
from tests.test_fuzz_gpu import REG_SEQUENCES

SEEDS = range(REG_SEQUENCES[1], REG_SEQUENCES[1] + REG_SEQUENCES[0])
WHOLE_BATCH = SS.EVAL_KINDS + SS.REFUSED        # a refused step ends with one rows evaluation of the whole batch
ONE_CONSTRAINT = ("dropin", "visuals")


@pytest.fixture(scope="module")
def scenes():
    return [SS.draw(seed) for seed in SEEDS]


def oracle_run(scenes):
    """the oracle's side of the fuzzer over the suite's range: every evaluation's rows -> evaluations"""
    n = 0
    for sc in scenes:
        model = SS.Model(sc)
        for st in sc.steps:
            if st["op"] in WHOLE_BATCH:
                model.evaluation(st["poses"])
                n += 1
            elif st["op"] in ONE_CONSTRAINT:
                model.rows(st["c"], st["poses"], model.draw(st["c"]))
                n += 1
    return n


def first_evaluations(sc):
    """(step of the first fused evaluation, of the first materialising one)"""
    fused = points = None
    for k, st in enumerate(sc.steps):
        if fused is None and st["op"] in SS.FUSED_PASS + ("solve",):
            fused = k
        if points is None and st["op"] in SS.POINTS_PASS + ("alloc_outputs",) + SS.REFUSED:
            points = k
    return fused, points


def test_the_range_is_whole_periods_and_every_arm_comes_twice(scenes):
    assert REG_SEQUENCES[0] % SS.PERIOD == 0
    arms = [sc.arm for sc in scenes]
    assert all(arms.count(a) >= 2 for a in SS.ARMS), arms
    assert all(sc.attempt <= 1 for sc in scenes), [sc.attempt for sc in scenes]
    assert all(len(sc.steps) == SS.STEPS for sc in scenes)


def test_every_op_kind_and_every_refused_kind_occurs(scenes):
    seen = {st["op"] for sc in scenes for st in sc.steps}
    assert seen == set(SS.OPS), set(SS.OPS) ^ seen
    for sampling in (True, False):
        kinds = {st["op"] for sc in scenes if sc.sampling == sampling for st in sc.steps if st["op"] in SS.REFUSED}
        assert kinds == set(SS.REFUSED), (sampling, set(SS.REFUSED) - kinds)
    assert not any(st["op"] in SS.ALL_POINTS_ONLY for sc in scenes if sc.sampling for st in sc.steps)
    # every source of blocks, every Jacobian subset, immediate and late fetches
    assert {st["src"] == "internal" for sc in scenes for st in sc.steps if st["op"] in ("assemble", "scatter")} == {True, False}
    assert {st["jac"] for sc in scenes for st in sc.steps if st["op"] in ("points", "points_f64")} == {(True, True), (True, False), (False, True), (False, False)}
    gaps = set()
    for sc in scenes:
        last = None
        for k, st in enumerate(sc.steps):
            if st["op"] == "rows":
                last = k
            elif st["op"] == "fetch":
                gaps.add(min(k - last, 3))
    assert gaps >= {1, 3}, gaps
    # a count between the evaluation of the internal blocks and their assembly
    assert any(a["op"] == "count_live_each" and b["op"] == "assemble" and b["src"] == "internal"
               for sc in scenes for a, b in zip(sc.steps, sc.steps[1:]))


def test_every_pose_class_is_the_first_evaluation_of_each_pass(scenes):
    firsts = [set(), set()]
    for sc in scenes:
        steps = first_evaluations(sc)
        assert None not in steps, sc.seed
        for p in range(2):
            cls = sc.steps[steps[p]]["cls"]
            assert cls == SS.first_classes(sc.seed)[p], (sc.seed, p, cls)
            firsts[p].add(cls)
    assert firsts[0] == firsts[1] == {"near", "half_out", "far", "yaw_pi"}, firsts
    assert any(st["cls"] == "previous" and st["poses"] is not None for sc in scenes for st in sc.steps)
    # a count is never taken at the last evaluation's poses
    for sc in scenes:
        last = None
        for st in sc.steps:
            if st["op"] in ("count_live", "count_live_each"):
                assert last is None or not np.array_equal(st["poses"], last)
            elif st["poses"] is not None:
                last = st["poses"]


def test_the_scenes_hold_what_the_issue_lists(scenes):
    planted, small = set(), 0
    for sc in scenes:
        planted.add(sc.counts[sc.planted_at])
        small += sc.small_at is not None and sc.counts[sc.small_at] < 64
        assert (sc.small_at is not None) == (sc.seed % 6 == 5)
        assert 4 <= len(sc.pairs) <= 8 and {k for p in sc.pairs for k in p} == {0, 1, 2}
        on_reference = [p for p in sc.pairs if p[0] == sc.reference]
        assert len(on_reference) >= (4 if sc.arm == "shared" else 3)
        assert any((b, a) in sc.pairs for a, b in sc.pairs), sc.pairs                      # a mirrored pair
        assert all(n > 0 for n in sc.residuals)
        assert all(len(p[2]) == n for p, n in zip(sc.points, sc.counts))
        assert sc.no_correspondence_cost in (0.0, 0.25) and sc.vps in (8, 16)
        if sc.sampling:
            assert sc.steps[-1]["op"] == "points" and sc.ratio in SS.RATIOS
    assert planted == set(SS.PLANTED) and small >= 2, (planted, small)
    assert {sc.private for sc in scenes if sc.sampling} == {True, False}
    assert {sc.use_esdf for sc in scenes} == {0, 1}
    assert {sc.sharded for sc in scenes} == {True, False}


def test_every_listed_refusal_is_one_and_every_valid_call_has_something_to_read(scenes):
    for sc in scenes:
        internal, rows, caller = "none", None, set()
        for k, st in enumerate(sc.steps):
            op = st["op"]
            if op == "normal" and st["into"] == "internal":
                internal = "blocks"
            elif op == "normal":
                caller.add(k)
            elif op == "cost" and st["into"] == "internal":
                internal = "none"
            elif op in SS.ALL_POINTS_ONLY:
                internal = "unknown"
            elif op == "rows":
                rows = st["want"]
            elif op == "fetch":
                assert rows is not None and all(h or not w for h, w in zip(rows, st["want"])), (sc.seed, k)
            elif op in ("assemble", "scatter"):
                assert internal == "blocks" if st["src"] == "internal" else st["src"] in caller, (sc.seed, k)
            elif op in ("refused_assemble", "refused_scatter"):
                assert internal == "none", (sc.seed, k)
            elif op == "refused_fetch":
                assert rows is not None and any(w and not h for h, w in zip(rows, st["want"])), (sc.seed, k)


def test_the_shared_arm_meets_the_documented_inputs_of_a_grouped_order_and_far_first_loads_nothing(scenes):
    for sc in scenes:
        steps = first_evaluations(sc)
        for p in range(2):
            loaded, shareable, everything = SS.order_inputs(sc, sc.steps[steps[p]]["poses"])
            if sc.arm == "shared":
                tiles = sum(-(-sc.counts[a] // SS.TILE) for a, _ in sc.pairs)
                assert tiles >= 16 and everything >= 16 * 1024, (sc.seed, tiles, everything)
                assert max(sc.counts) < 5 * 1024 * 2             # every fused tile is one 1024-point tile, as restated
                assert shareable >= 0.3 * loaded and loaded >= 0.75 * everything, (sc.seed, p, loaded, shareable, everything)
            elif sc.arm == "far_first":
                assert loaded == 0, (sc.seed, p, loaded)
            elif sc.arm == "near_first":
                assert loaded > 0, (sc.seed, p)


def test_the_oracle_side_runs_every_evaluation(scenes):
    assert oracle_run(scenes) >= 8 * len(scenes)


@pytest.mark.skipif(not ref_reg.available(), reason="oracle/_ref/libref_reg.so not built (needs the reference's sources)")
def test_the_sampling_model_is_the_reference_cost_function_called_in_the_same_order(scenes):
    checked = 0
    for sc in scenes:
        if not sc.sampling:
            continue
        model = SS.Model(sc)

        def submap(k):
            sm = sc.submaps[k]
            R = ref_reg.Submap(k, np.zeros(4), sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight,
                               sm.esdf_distance, sm.esdf_observed, use_esdf_distance=bool(sc.use_esdf))
            R.set_points(ref_reg.POINTS_VOXELS, *sc.points[k])
            return R
        shared = [submap(k) for k in range(3)]
        # a private engine: a point-set copy of the constraint's own (its WeightedSampler starts at 5489, as PRIVATE_SEED)
        refs = [ref_reg.RegistrationCostFunction(submap(a) if sc.private else shared[a], shared[b], ref_reg.POINTS_VOXELS,
                                                 sampling_ratio=sc.ratio, no_correspondence_cost=sc.no_correspondence_cost,
                                                 use_esdf_distance=bool(sc.use_esdf)) for a, b in sc.pairs]
        assert [r.num_residuals() for r in refs] == sc.residuals

        def one(c, poses):
            a, b = sc.pairs[c]
            ok, r, jo, je = refs[c].Evaluate(poses[a], poses[b])
            ok0, r0, jo0, je0 = model.rows(c, poses, model.draw(c))
            assert ok == ok0 and np.array_equal(r, r0) and np.array_equal(jo, jo0) and np.array_equal(je, je0), (sc.seed, c)
        for st in sc.steps:
            if st["op"] in WHOLE_BATCH:
                for c in range(len(sc.pairs)):
                    one(c, st["poses"])
                checked += 1
            elif st["op"] in ONE_CONSTRAINT:
                one(st["c"], st["poses"])
                checked += 1
    assert checked >= 8
