"""A short run of each differential fuzzer (profiles/fuzz_*.py: random configurations / poses / clusters /
sampling set-ups against the oracles, exact comparisons) inside the suite, so that the driver's GPU run
exercises them too.  Fixed seeds: deterministic.  The long runs are recorded in profiles/README.md."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (seeds, first) of the two map-product fuzzers: tests/test_fuzz_map_cpu.py checks the generator over exactly these
MAP_LAYERS = (36, 300)
MAP_MESHES = (60, 300)
# (seeds, first) of the ESDF fuzzer: tests/test_esdf_cpu.py holds the restatement to the queue over exactly these draws
ESDF = (24, 300)
# (seeds, first) of the layer readers' fuzzer: tests/test_fuzz_readers_cpu.py checks the generator over exactly these.  The
# count is the largest whose restatement side stays within 1.5 times that of MAP_LAYERS (profiles/README.md)
READERS = (144, 300)
# (seeds, first) of the pose-graph fuzzer: tests/test_fuzz_pose_graph_cpu.py checks the generator over exactly these.  The
# count follows the readers' rule (profiles/README.md); the size schedule has a period of 24 seeds
POSE_GRAPH = (32, 300)
# (seeds, first) of the registration batch's sequence fuzzer: tests/test_fuzz_reg_sequences_cpu.py checks the generator over
# exactly these.  The schedule has a period of 12 seeds; the readers' rule would hold 72, two periods keep the test at a
# few seconds (profiles/README.md)
REG_SEQUENCES = (24, 300)


def _load(script):
    spec = importlib.util.spec_from_file_location(script, os.path.join(ROOT, "profiles", script + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(script, seeds, first):
    mod = _load(script)
    old = {k: os.environ.get(k) for k in ("SEEDS", "FIRST")}
    os.environ["SEEDS"], os.environ["FIRST"] = str(seeds), str(first)
    try:
        return mod.main()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_tsdf_random_configurations_bit_identical_to_the_oracle():
    """fast + merged integrators in the reproducible mode, merged in the racing mode: 25 random configurations"""
    assert _run("fuzz_tsdf", 25, 300) == 0


def test_racing_tsdf_random_configurations_replay_as_legal_interleavings():
    """the racing (default) mode by trace and replay: 12 random integrator configurations x 4 scans (unorganised and
    organised clouds incl. ragged tiles, counted and uncounted kernels, colours, free-space scans); the long runs
    (1360 scans, 59 M exchanges, 0 violations) are recorded in profiles/README.md"""
    assert _run("fuzz_replay", 12, 300) == 0


def test_reg_random_constraints_equal_the_oracle():
    """drop-in f64 rows, batched f32 rows, fused sums, voxel-point and isosurface producers: 60 random submap pairs"""
    assert _run("fuzz_reg", 60, 300) == 0


def test_overlap_random_clusters_equal_the_oracle():
    assert _run("fuzz_overlap", 40, 300) == 0


def test_sampling_random_setups_follow_the_oracles_streams():
    assert _run("fuzz_sampling", 30, 300) == 0


def test_reg_at_128_cubed_every_row_equal_and_fused_sums_close():
    """four 128^3 city submaps, twelve constraints, two pose sets per seed: every materialised row exact, fused
    sums within 2e-6 (this is the fuzzer that made the fused kernel share the reference's interpolated value)"""
    assert _run("fuzz_reg_large", 3, 300) == 0


def test_sampling_at_128_cubed_follows_the_oracles_streams():
    assert _run("fuzz_sampling_large", 3, 300) == 0


def test_sharded_evaluation_is_the_single_batch_bit_for_bit():
    """random pose graphs sharded over 1-8 contexts by LPT / contiguous / arbitrary placements: fused buffer,
    per-constraint blocks and the scatter -> int64 sum -> assemble route equal the single batch's bits (25 graphs)"""
    assert _run("fuzz_multi", 25, 700) == 0


def test_map_layers_random_scenes_bit_identical_to_the_restatements():
    """the projected map into an empty and a non-empty layer, transformLayer, queries and the evaluation on the projected
    map: grid-aligned poses, dyadic voxel sizes, planted validity thresholds, block boxes far from the origin"""
    assert _run("fuzz_map_layers", *MAP_LAYERS) == 0


def test_map_meshes_random_scenes_bit_identical_to_the_restatements():
    """the combined, submap and separated meshes at the drawn min_weight, each welded at two thresholds from 1e-10 to
    four times the scene's extent (thousands of soup vertices into one key)"""
    assert _run("fuzz_map_meshes", *MAP_MESHES) == 0


def test_layer_readers_random_scenes_bit_identical_to_the_restatements():
    """views of the live layer and of a finished submap (both launches), scan-to-map registration (evaluate, refine) and
    scan localisation (evaluate_map, score_poses, localize) on scenes far from the origin, with grid-aligned poses, empty
    and duplicated submaps, and voxels that hold NaN, +-inf, -0.0, denormals and negative weights; a NaN equals a NaN"""
    assert _run("fuzz_layer_readers", *READERS) == 0


def test_pose_graph_random_graphs_bit_identical_to_the_restatements():
    """random block matrices (bad pivots among them), edges-only graphs and registration lists over a ring of 12 submaps:
    both Cholesky routes, the three orderings, both covariance routes and the slabs against the sequential restatements,
    every bit; sparse in natural order next to dense as numbers (the sign of a zero may differ)"""
    assert _run("fuzz_pose_graph", *POSE_GRAPH) == 0


def test_esdf_random_submaps_bit_identical_to_the_restatement_and_close_to_the_queue():
    """shell-observed and carved submaps, random max / default / min distances: both ESDF layers the bits of tests/esdf_ref.py,
    and the queue's contract (masks, fixed band, signs, never above, within 4 mm, fixed-point residual)"""
    assert _run("fuzz_esdf", *ESDF) == 0


def test_one_long_lived_registration_batch_through_random_call_sequences():
    """14 calls per batch handle -- every rows entry point, kept rows and late fetches, fused blocks and costs into the
    internal and the caller's arrays, assemblies from both, live counts in between, drop-in and visuals evaluations,
    refused calls of every kind, a placement trial and a pose-graph solve -- each held to the oracle's rows and, all-points
    batches, to the same call on a fresh handle, bit for bit; sampling batches to the oracle's engines draw for draw.  Both
    launch orders must have been met in either pass: a grouped order is what later poses could disagree with"""
    rc, summary = _load("fuzz_reg_sequences").run(*REG_SEQUENCES)
    assert rc == 0
    for p, name in enumerate(("fused pass", "materialising pass")):
        assert summary["grouped"][p] > 0 and summary["not_grouped"][p] > 0, (name, summary)
