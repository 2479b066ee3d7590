"""The pose-graph fuzzer (profiles/fuzz_pose_graph.py) kept honest without a GPU, the counterpart of
tests/test_fuzz_readers_cpu.py: the product's host pattern code (vgx_pose_graph_tile_pattern: no context, no HIP call)
against the restatement over 2160 random structures of the generator's families under all three orderings; then, over
exactly the seed range tests/test_fuzz_gpu.py runs, the scene generator (profiles/fuzz_pose_graph_scene.py) and the
restatements alone must draw every class and reach every path of the kernels the issue names at least twice, stay under
the two caps, and agree with each other as numbers under the natural order.

Where a kernel path is named here it is derived from the restated tile lists (fuzz_pose_graph_scene.structure_features,
chunk_features), not from a run of the kernel.  With I >= J in every update triple, a partial last tile row that is a
triple's J is its I as well: "its J" and "both" are one case, partial_row_is_I_and_J."""
import importlib.util
import os

import numpy as np
import pytest

from profiles import fuzz_pose_graph_scene as PS
from tests import pose_graph_ref as ref
from tests import pose_graph_sparse_ref as sref
from tests.test_fuzz_gpu import POSE_GRAPH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuzzer(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "profiles", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FP = _fuzzer("fuzz_pose_graph")
N_PATTERNS = 2160                            # ten rounds of 9 families x 24 size slots


# ---- the product's host code against the restatement ----------------------------------------------------------------
def test_host_tile_pattern_is_the_restatement_on_random_structures_under_every_ordering():
    from voxgraph_amd import capi
    capi.load()
    families, classes = set(), set()
    for k in range(N_PATTERNS):
        family, n, pairs, given = PS.pattern_case(k)
        families.add(family)
        classes.add(PS.ROW_SCHEDULE[(k // len(PS.FAMILIES)) % len(PS.ROW_SCHEDULE)])
        for ordering in PS.ORDERINGS:
            order, tiles = capi.tile_pattern(n, pairs, ordering, given if ordering == sref.GIVEN else None)
            order0 = sref.make_order(n, pairs, ordering, given)
            assert order.tolist() == order0, (k, family, n, ordering)
            assert [tuple(t) for t in tiles.tolist()] == sref.tile_pattern(n, pairs, order0)[1], (k, family, n, ordering)
    assert families == set(PS.FAMILIES) and classes == set(PS.ROW_CLASSES)


# ---- the generator and the restatements over the suite's seeds ------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    """the restatements' side of fuzz_pose_graph over the suite's range (what profiles/README.md times)"""
    seeds, first = POSE_GRAPH
    out = []
    for seed in range(first, first + seeds):
        sc = PS.scene(seed)
        m, g = sc.matrix, sc.graph
        clean, bad = FP.matrix_reference(m)
        solved, cw = FP.graph_reference(g), FP.covariance_reference(g)
        feats = {"matrix": set(m.features), "graph": set(), "chunks": set()}
        if g.nfree and g.edges:
            pos, _ = ref.free_positions(g.n, g.constant)
            feats["graph"], _, _ = PS.structure_features(g.nfree, sref.joined_free_pairs(pos, (), g.edges), solved["keep"]["order"])
        if cw is not None:
            feats["chunks"] = PS.chunk_features(g.nf, cw["l_tiles"], cw["place"], g.cov_pairs)
        out.append(dict(sc=sc, clean=clean, bad=bad, solved=solved, cw=cw, feats=feats))
    return out


def _count(run, predicate):
    return sum(1 for r in run if predicate(r))


def test_the_same_seed_gives_the_same_scene():
    a, b = PS.scene(POSE_GRAPH[1] + 3), PS.scene(POSE_GRAPH[1] + 3)
    assert PS.describe(a) == PS.describe(b) != PS.describe(PS.scene(POSE_GRAPH[1] + 4))
    assert FP.same_bits(a.matrix.A, b.matrix.A) and FP.same_bits(a.matrix.B, b.matrix.B) and FP.same_bits(a.graph.poses0, b.graph.poses0)
    assert all(FP.same_bits(x.A, y.A) for x, y in zip(a.matrix.bad, b.matrix.bad)) and len(a.matrix.bad) == 2
    assert all(x[:2] == y[:2] and FP.same_bits(x[4], y[4]) for x, y in zip(a.graph.edges, b.graph.edges))
    assert a.registration.pairs == b.registration.pairs and FP.same_bits(a.registration.poses0, b.registration.poses0)


def test_every_class_family_and_ordering_is_drawn_at_least_twice(run):
    for name, of, values in (("matrix size class", lambda r: r["sc"].matrix.size_class, PS.ROW_CLASSES), ("pattern family", lambda r: r["sc"].matrix.family, PS.FAMILIES),
                             ("graph size class", lambda r: r["sc"].graph.size_class, PS.NODE_CLASSES), ("topology", lambda r: r["sc"].graph.topology, PS.TOPOLOGIES),
                             ("graph ordering", lambda r: r["sc"].graph.ordering, PS.ORDERINGS), ("registration ordering", lambda r: r["sc"].registration.ordering, PS.ORDERINGS),
                             ("right-hand sides in place", lambda r: r["sc"].matrix.in_place, (False, True))):
        for v in values:
            assert _count(run, lambda r: of(r) == v) >= 2, (name, v)
    assert {r["sc"].matrix.m for r in run} <= set(PS.M_VALUES) and len({r["sc"].matrix.m for r in run}) >= 6
    for cls, (lo, hi) in PS.ROW_CLASSES.items():
        assert all(lo <= r["sc"].matrix.rows <= hi for r in run if r["sc"].matrix.size_class == cls)
    for cls, (lo, hi) in PS.NODE_CLASSES.items():
        assert all(lo <= r["sc"].graph.n <= hi for r in run if r["sc"].graph.size_class == cls)
    wide = [r["sc"].graph for r in run if r["sc"].graph.size_class == "wide"]
    assert all(g.options["max_num_iterations"] <= 3 for g in wide) and max(r["sc"].graph.options["max_num_iterations"] for r in run) > 8
    # full, odometry and closure information; constant nodes with and without node 0; repeated pairs in both directions
    graphs = [r["sc"].graph for r in run if r["sc"].graph.edges]
    assert _count(run, lambda r: any(np.count_nonzero(e[4]) > 4 for e in r["sc"].graph.edges)) >= 2
    assert sum(1 for g in graphs if g.constant[0]) >= 2 and sum(1 for g in graphs if not g.constant[0]) >= 2
    assert sum(1 for g in graphs if len({(e[0], e[1]) for e in g.edges}) < len(g.edges)) >= 2
    assert sum(1 for g in graphs if any((e[1], e[0]) in {(f[0], f[1]) for f in g.edges} for e in g.edges)) >= 2
    assert _count(run, lambda r: not r["sc"].graph.cov_pairs and r["sc"].graph.n > 1) >= 1
    assert _count(run, lambda r: any(a == b for a, b in r["sc"].graph.cov_pairs)) >= 2


def test_every_named_path_of_the_kernels_is_reached_at_least_twice(run):
    both = lambda r: r["feats"]["matrix"] | r["feats"]["graph"]  # noqa: E731
    for name in ("pure_fill_tile", "fill_of_fill", "empty_column", "column_count_odd", "column_count_even", "row_count_odd", "row_count_even",
                 "column_over_16_tiles", "row_over_16_tiles", "partial_row_is_I_alone", "partial_row_is_I_and_J"):
        assert _count(run, lambda r: name in both(r)) >= 2, name
    # the wide matrix scenes are where a column has more than 16 tiles under its diagonal tile
    assert _count(run, lambda r: r["sc"].matrix.size_class == "wide" and "column_over_16_tiles" in r["feats"]["matrix"]) >= 2
    for name in ("forward_starts_past_panel_0", "backward_skips_a_tile"):
        assert _count(run, lambda r: name in r["feats"]["chunks"]) >= 2, name
    assert _count(run, lambda r: r["cw"] is not None and r["cw"]["stats"]["n_slabs"] >= 2) >= 2
    assert _count(run, lambda r: r["cw"] is not None and r["cw"]["stats"]["n_slabs"] >= 2 and r["cw"]["sparse"] is not None) >= 2
    # the damping's lower clip, 1e-6, decides a step: a diagonal of H below it, a gradient there, an iteration that factorises
    clipped = lambda r: bool(r["solved"] and r["solved"]["dense"][2] and r["solved"]["dense"][2][0]["step_norm"] > 0 and r["cw"] is not None  # noqa: E731
                             and ((np.diag(r["cw"]["H"]) < 1e-6) & (np.diag(r["cw"]["H"]) > 0) & (r["cw"]["g"] != 0)).any())
    assert _count(run, clipped) >= 2
    histories = [r["solved"]["dense"][2] for r in run if r["solved"]]
    rejected = lambda h: any(not x["accepted"] and not x["factorization_failed"] and x["trial_cost"] != 0.0 for x in h)  # noqa: E731
    assert sum(1 for h in histories if rejected(h) and any(x["accepted"] for x in h)) >= 2
    assert _count(run, lambda r: r["solved"] and PS.wrapped_yaw_errors(r["sc"].graph) > 0) >= 2
    for reason in ("parameter_tolerance", "function_tolerance", "max_iterations"):
        assert _count(run, lambda r: r["solved"] and r["solved"]["dense"][1]["termination"] == reason) >= 2, reason
        assert _count(run, lambda r: r["solved"] and r["solved"]["sparse"][1]["termination"] == reason) >= 2, reason


def test_every_bad_pivot_kind_is_drawn_and_refused_by_both_restatements(run):
    variants = [(v, b) for r in run for v, b in zip(r["sc"].matrix.bad, r["bad"])]
    for kind in PS.BAD_KINDS:
        assert sum(1 for v, b in variants if v.kind == kind and b is None) >= 2, kind
    assert sum(1 for v, _ in variants if v.last_tile) >= 2                # rows of the last partial tile
    for v, _ in variants:
        if v.kind == "fill":                                               # the pivot is bad only through the fill tile (2, 1)
            with pytest.raises(ref.NotPositiveDefinite) as e:
                ref.cholesky(v.A)
            assert e.value.args[0] == 128 and 31.0 < v.A[4, 4] < 32.0 and np.diag(v.A).min() > 0
    values = [float(v.A[v.row, v.row]) for v, _ in variants if v.kind == "nonpositive"]
    assert all(x <= 0 for x in values)


def test_the_two_caps_hold(run):
    """scenes whose free part fits one tile: at most a quarter of the graph scenes; refused or degenerate scenes (a graph of
    constant nodes alone or without an edge, a rank-deficient graph, a matrix scene with bad pivots): at most one in five"""
    n = len(run)
    assert 4 * _count(run, lambda r: r["sc"].graph.nfree <= PS.NODES_PER_TILE) <= n
    no_solve = _count(run, lambda r: r["solved"] is None)
    deficient = _count(run, lambda r: r["cw"] is not None and (r["cw"]["dense"] is None or r["cw"]["sparse"] is None))
    bad = _count(run, lambda r: bool(r["sc"].matrix.bad))
    assert no_solve >= 2 and deficient >= 2 and bad >= 2
    assert _count(run, lambda r: r["sc"].graph.all_constant and r["sc"].graph.edges) >= 1
    assert 5 * (no_solve + deficient) <= n and 5 * bad <= n and 5 * (no_solve + deficient + bad) <= 2 * n
    # both kinds of the rank-deficient sub-class, and both restatements raise on them
    kinds = {r["sc"].graph.lonely is None for r in run if r["sc"].graph.rank_deficient_by_design}
    assert kinds == {False, True}
    assert all(r["cw"] is None or (r["cw"]["dense"] is None and r["cw"]["sparse"] is None) for r in run if r["sc"].graph.rank_deficient_by_design)


def test_under_the_natural_order_the_sparse_restatement_gives_the_dense_restatements_numbers(run):
    """factor and solve (every matrix scene is in natural order), history and covariance blocks (the graph scenes drawn
    with the natural order): only the sign of a zero may differ"""
    solves = blocks = 0
    for r in run:
        m, c = r["sc"].matrix, r["clean"]
        assert np.array_equal(sref.to_dense(c["L"], m.n), c["Ld"]) and np.array_equal(c["x"], c["xd"]) and np.array_equal(c["X"], c["Xd"]), m.seed
        g = r["sc"].graph
        if g.ordering != sref.NATURAL:
            continue
        if r["solved"]:
            assert FP.compare_solve("sparse next to dense", r["solved"]["sparse"], r["solved"]["dense"], FP.same_numbers) is None, g.seed
            solves += 1
        if r["cw"] is not None and r["cw"]["dense"] is not None:
            assert np.array_equal(r["cw"]["sparse"], r["cw"]["dense"]), g.seed
            blocks += 1
    assert solves >= 4 and blocks >= 4


def test_the_comparators_report_a_flipped_bit_a_zero_sign_and_a_changed_count(run):
    r = next(r for r in run if r["solved"] and len(r["solved"]["dense"][2]) >= 2)
    x, s, hist = r["solved"]["dense"]
    copy = lambda: (x.copy(), dict(s), [dict(h) for h in hist])  # noqa: E731
    assert FP.compare_solve("s", copy(), (x, s, hist)) is None
    got = copy()
    got[0].view(np.uint64)[1, 2] ^= 1
    assert "poses" in FP.compare_solve("s", got, (x, s, hist))
    for key in FP.KEYS:
        got = copy()
        got[2][1][key] = np.nextafter(got[2][1][key], np.inf)
        assert key in FP.compare_solve("s", got, (x, s, hist))
    got = copy()
    got[2][0]["accepted"] ^= 1
    assert "accepted" in FP.compare_solve("s", got, (x, s, hist))
    got = copy()
    got[1]["num_iterations"] += 1
    assert "after" in FP.compare_solve("s", got, (x, s, hist))
    a, b = np.zeros(4), np.array([0.0, 0.0, -0.0, 0.0])
    assert "1 of 4" in FP.compare_arrays("z", a, b) and FP.compare_arrays("z", a, b, FP.same_numbers) is None
    assert "shape" in FP.compare_arrays("z", a, np.zeros(5)) and FP.compare_arrays("z", np.array([np.nan]), np.array([np.nan])) is None


def test_the_restated_cholesky_in_strips_is_its_one_statement_per_k_bit_for_bit():
    """tests/pose_graph_ref.cholesky walks strips of 64 columns so that this file's run stays affordable; the statement it
    restates is `A[k + 1:, k + 1:] -= outer(column k, column k)` for k ascending, written out here -- with a NaN below the
    diagonal and a bad pivot past the first strip as well"""
    import math

    def statement(A):
        A = np.array(A, np.float64)
        for k in range(A.shape[0]):
            if not (A[k, k] > 0.0) or math.isinf(A[k, k]):
                raise ref.NotPositiveDefinite(k)
            A[k, k] = math.sqrt(A[k, k])
            A[k + 1:, k] = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
        return np.tril(A)

    rng = np.random.default_rng(4)
    for n in (1, 2, 63, 64, 65, 129, 300):
        M = rng.normal(0, 1, (n, n))
        A = M @ M.T + n * np.eye(n)
        assert FP.same_bits(ref.cholesky(A), statement(A)), n
        if n >= 129:
            for row, col, value in ((100, 100, -1.0), (120, 70, np.nan), (128, 128, np.inf)):
                B = A.copy()
                B[row, col] = B[col, row] = value
                with np.errstate(all="ignore"), pytest.raises(ref.NotPositiveDefinite) as a:
                    ref.cholesky(B)
                with np.errstate(all="ignore"), pytest.raises(ref.NotPositiveDefinite) as b:
                    statement(B)
                assert a.value.args == b.value.args and a.value.args[0] >= 100
