"""The tile-sparse pose-graph solver on the device (include/voxgraph_amd.h, "Pose graph: the tile-sparse solver") against
the dense solver this project tests bit for bit, and against its own restatement (tests/pose_graph_sparse_ref.py):
vgx_block_spd_solve next to vgx_dense_spd_solve on one matrix, bad pivots, whole solves in sparse mode next to dense
mode on a second handle, orderings, a graph past the dense limit (nf = 16796), switching and refusals.

"Equal" against the DENSE solver is np.array_equal -- the two can differ in the sign of a zero; against the sparse
restatement it is every bit."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import pose_graph_ref as ref
from tests import pose_graph_sparse_ref as sref
from tests.test_pose_graph_gpu import KEYS, EdgesOnly, Ring, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi
    capi.load()
    return capi


@pytest.fixture(scope="module")
def ctx(capi):
    import torch
    c = capi.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _refused(capi, ctx, code, call):
    with pytest.raises(capi.VgxError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


# ---- 1: the factorisation on a caller's matrix ----------------------------------------------------------------------
def _break_chain(pairs, tiles):
    """drop the pairs that join tile t to tile t + 1, for t in `tiles`"""
    return [(i, j) for i, j in pairs if not (i // 16 != j // 16 and j // 16 in tiles)]


def block_scenes():
    """n -> (block rows, pairs): one partial tile; the tile edge; an arrow (tiles (1, 0), (2, 0) stored, (2, 1) pure fill); a
    band with a closure whose fill runs along tile row 4; 18 panels, the columns of tiles 7, 8 and 12 empty below the diagonal;
    an arrowhead of 19 tile rows (the last 4 rows wide) whose fill stores all 190 tiles: 18 and 17 tiles below the diagonal in
    columns 0 and 1, 17 and 18 left of it in the last two rows -- more than the 16 a pass of the substitutions takes"""
    return {4: (1, []), 64: (16, sref.chain_pairs(16)), 68: (17, sref.chain_pairs(17)), 132: (33, [(i, 0) for i in range(1, 33)]),
            300: (75, sref.chain_pairs(75, closures=[(74, 3)])),
            1100: (275, _break_chain(sref.chain_pairs(275), (3, 7, 8, 12)) + [(270, 20)]),
            1156: (289, [(i, 0) for i in range(1, 289)])}


def scattered(index, tiles, n):
    return sref.to_dense({(int(i), int(j)): T for (i, j), T in zip(index, tiles)}, n)


@pytest.mark.parametrize("n", sorted(block_scenes()))
def test_block_spd_solve_equals_the_dense_solve_and_is_the_restatement_bit_for_bit(capi, ctx, n):
    rows, pairs = block_scenes()[n]
    m = sref.block_matrix(rows, pairs, seed=n)
    x, stats, index, tiles = capi.block_spd_solve(ctx, rows, m["bi"], m["bj"], m["values"], m["b"])
    xd, Ld = capi.dense_spd_solve(ctx, m["A"], m["b"])
    h_keys, l_tiles = sref.tile_pattern(rows, m["pairs"], list(range(rows)))
    x0, L0 = sref.spd_solve(sref.to_tiles(m["A"], [t for t in l_tiles if t in h_keys]), n, l_tiles, m["b"])
    L = scattered(index, tiles, n)
    nT = (n + 63) // 64
    print(f"n {n}: {stats}; max |L - dense L| {np.abs(L - Ld).max():.3e}, max |x - dense x| {np.abs(x - xd).max():.3e}")
    assert [tuple(t) for t in index.tolist()] == l_tiles
    assert stats["n_l_tiles"] == len(l_tiles) and stats["n_update_triples"] == len(sref.update_triples(l_tiles))
    assert stats["n_panels"] == nT and stats["n_launches"] == sref.launches(l_tiles) and stats["n_free_variables"] == n
    assert np.array_equal(L, Ld) and np.array_equal(x, xd)
    assert same_bits(L, sref.to_dense(L0, n)) and same_bits(x, x0)
    for key, T in zip(index.tolist(), tiles):                            # ... tile by tile: zeros above the diagonal and past the matrix
        assert same_bits(T, L0[tuple(key)])
    if n == 132:
        assert l_tiles == [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)] and (2, 1) not in h_keys and np.abs(L[128:, 64:128]).max() > 0
    if n == 300:
        assert {(4, 1), (4, 2)} == set(l_tiles) - h_keys and (4, 0) in h_keys
    if n == 1100:
        assert nT == 18 and stats["n_launches"] < 3 * 17 + 1 - 4 and len(l_tiles) < nT * (nT + 1) // 2 // 3
    if n == 1156:                                                        # every tile stored: the dense solver's history, so its bits
        below = [len(rows_of) - 1 for _, rows_of in sorted(sref.columns_of(l_tiles).items())]
        assert nT == 19 and len(l_tiles) == 190 and below == list(range(18, -1, -1)) and max(below) > 16
        assert same_bits(L, Ld) and same_bits(x, xd)


def test_block_spd_solve_refuses_what_it_cannot_take(capi, ctx):
    m = sref.block_matrix(17, sref.chain_pairs(17), seed=1)
    bi, bj, v = m["bi"], m["bj"], m["values"]
    twice = (np.append(bi, bi[-1]), np.append(bj, bj[-1]), np.concatenate([v, v[-1:]]))
    above = (np.append(bi, 2), np.append(bj, 9), np.concatenate([v, v[-1:]]))
    outside = (np.append(bi, 17), np.append(bj, 0), np.concatenate([v, v[-1:]]))
    for (i, j, vals), word in ((twice, "twice"), (above, "above the diagonal"), (outside, "out of range")):
        assert word in _refused(capi, ctx, capi.ERR_INVALID, lambda: capi.block_spd_solve(ctx, 17, i, j, vals, m["b"], want_factor=False))


# ---- 2: bad pivots --------------------------------------------------------------------------------------------------
def _blocks(A, m):
    return np.array([A[4 * i:4 * i + 4, 4 * j:4 * j + 4] for i, j in zip(m["bi"], m["bj"])])


def _both_refuse(capi, ctx, m, A):
    with pytest.raises(ref.NotPositiveDefinite):
        ref.cholesky(A)
    for call in (lambda: capi.dense_spd_solve(ctx, A, m["b"]),
                 lambda: capi.block_spd_solve(ctx, m["n_block_rows"], m["bi"], m["bj"], _blocks(A, m), m["b"])):
        assert "not positive definite" in _refused(capi, ctx, capi.ERR_NOT_POSITIVE_DEFINITE, call)


def test_bad_pivot_in_a_diagonal_tile_and_inf_on_the_diagonal_are_reported_where_the_dense_solve_reports_them(capi, ctx):
    rows, pairs = block_scenes()[300]
    m = sref.block_matrix(rows, pairs, seed=300)
    for row, value in ((70, -1e6), (200, np.inf), (299, np.nan), (0, 0.0)):
        A = m["A"].copy()
        A[row, row] = value
        _both_refuse(capi, ctx, m, A)
    x, _, index, tiles = capi.block_spd_solve(ctx, rows, m["bi"], m["bj"], m["values"], m["b"])      # nothing sticks
    xd, Ld = capi.dense_spd_solve(ctx, m["A"], m["b"])
    assert np.array_equal(x, xd) and np.array_equal(scattered(index, tiles, 300), Ld)


def test_bad_pivot_that_arrives_through_a_fill_tile_is_reported_where_the_dense_solve_reports_it(capi, ctx):
    """The arrow: node 0 with the identity, every other node d I with the block I towards node 0.  The Schur complement
    on nodes 1..32 is d I - 1 1^T (x I4): its pivots fall, and the last node's -- alone in tile 2 -- is positive exactly
    when d > 32.  With 31 < d < 32 it is negative only through the 16 nodes of tile 1, whose products reach it through
    the fill tile (2, 1): without that tile's update the pivot would be d - 16 > 0."""
    rows, pairs = block_scenes()[132]
    m = sref.block_matrix(rows, pairs, seed=0)

    def arrow(d):
        A = np.zeros((132, 132))
        A[:4, :4] = np.eye(4)
        for i in range(1, 33):
            A[4 * i:4 * i + 4, 4 * i:4 * i + 4] = d * np.eye(4)
            A[4 * i:4 * i + 4, :4] = A[:4, 4 * i:4 * i + 4] = np.eye(4)
        return A

    bad = arrow(31.5)
    with pytest.raises(ref.NotPositiveDefinite) as e:
        ref.cholesky(bad)
    assert e.value.args[0] == 128                                        # the first pivot of tile 2
    _both_refuse(capi, ctx, m, bad)
    good = arrow(32.5)
    x, _, index, tiles = capi.block_spd_solve(ctx, rows, m["bi"], m["bj"], _blocks(good, m), m["b"])
    xd, Ld = capi.dense_spd_solve(ctx, good, m["b"])
    assert np.array_equal(x, xd) and np.array_equal(scattered(index, tiles, 132), Ld) and Ld[128, 128] > 0


# ---- 3: whole solves, sparse mode in natural order next to dense mode on a second handle ----------------------------
SUMMARY_KEYS = ("termination_type", "termination_reason", "num_iterations", "num_successful_steps", "num_full_evaluations",
                "num_cost_evaluations", "num_factorization_failures", "num_free_nodes", "initial_cost", "final_cost")


def _solved(pg, poses0, **kw):
    x, s = pg.optimize(poses0, max_solver_time_in_seconds=600.0, **kw)
    return x, s, pg.history(), pg.download_system()


def _assert_same_solve(a, b):
    (xa, sa, ha, (Ha, ga)), (xb, sb, hb, (Hb, gb)) = a, b
    assert np.array_equal(xa, xb)
    assert [sa[k] for k in SUMMARY_KEYS] == [sb[k] for k in SUMMARY_KEYS] and sa["termination"] == sb["termination"]
    assert len(ha) == len(hb) >= 1
    for k in KEYS + ("accepted", "factorization_failed"):
        assert np.array_equal([h[k] for h in ha], [h[k] for h in hb]), k
    assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb) and np.abs(Ha).max() > 0


def _sparse_next_to_dense(capi, ctx, scene, poses0, **kw):
    dense, sparse = scene.graph(capi, ctx), scene.graph(capi, ctx)
    sparse.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE)
    a, b = _solved(dense, poses0, **kw), _solved(sparse, poses0, **kw)
    stats = sparse.structure()
    _refused(capi, ctx, capi.ERR_INVALID, dense.structure)
    assert sparse.order().tolist() == dense.order().tolist() == list(range(a[1]["num_free_nodes"]))
    dense.destroy()
    sparse.destroy()
    _assert_same_solve(a, b)
    return a, stats


@pytest.fixture(scope="module")
def mixed(capi):
    return EdgesOnly(capi, ref.mixed_graph(80, ref.MIXED_SEED))


def test_mixed_graph_in_sparse_mode_solves_as_dense_mode_does(capi, ctx, mixed):
    (x, s, hist, _), stats = _sparse_next_to_dense(capi, ctx, mixed, mixed.g["poses0"], exclude_registration_constraints=1, **ref.MIXED_SOLVE)
    accepted = [h["accepted"] for h in hist]
    assert stats["n_free_variables"] == 308 and stats["n_panels"] == 5 and 1 in accepted and 0 in accepted[:-1]
    assert np.abs(mixed.g["poses0"][:, 3]).max() > 2 * np.pi >= 2 * np.abs(x[:, 3]).max()


@pytest.fixture(scope="module")
def ring20(capi, ctx):
    r = Ring(capi, ctx, 20)
    yield r
    r.destroy()


@pytest.mark.parametrize("exclude", (False, True))
def test_ring_of_20_in_sparse_mode_solves_as_dense_mode_does(capi, ctx, ring20, exclude):
    (x, s, _, _), stats = _sparse_next_to_dense(capi, ctx, ring20, ring20.g["poses0"], exclude_registration_constraints=int(exclude))
    assert stats["n_free_variables"] == 76 and stats["n_l_tiles"] == 3 and s["num_successful_steps"] >= 1


class AssemblyScene:
    """ref.assembly_scene with what _sparse_next_to_dense asks of a scene"""

    def __init__(self, capi, ctx):
        self.g, ring6, self.pairs, self.poses = ref.assembly_scene()
        self.submaps = [H.gpu_submap(capi, ctx, sm, i) for i, sm in enumerate(ref.ring_submaps(ring6))]
        for s in self.submaps:
            s.extract_voxel_points()
        cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
        self.cfs = [capi.RegistrationCostFunction(ctx, self.submaps[a], self.submaps[b], cfg) for a, b in ref.ASSEMBLY_SUBMAP_PAIRS]
        self.batch = capi.RegistrationBatch(ctx, self.cfs, self.pairs)
        self.edges = [capi.pose_graph_edge(*e) for e in self.g["edges"]]

    def graph(self, capi, ctx):
        pg = capi.PoseGraph(ctx, 80, self.g["constant"])
        pg.set_registration(self.batch)
        pg.set_edges(self.edges)
        return pg

    def destroy(self):
        for o in [self.batch] + self.cfs + self.submaps:
            o.destroy()


def test_assembly_scene_in_sparse_mode_solves_as_dense_mode_does(capi, ctx):
    scene = AssemblyScene(capi, ctx)
    (_, s, _, (Hd, _)), stats = _sparse_next_to_dense(capi, ctx, scene, scene.poses, max_num_iterations=4)
    scene.destroy()
    assert Hd.shape == (308, 308) and s["num_full_evaluations"] >= 2 and stats["n_h_tiles"] > 5


# ---- 4: orderings ---------------------------------------------------------------------------------------------------
def _assert_is_the_restatement(x, s, hist, restated):
    x0, s0, hist0 = restated
    assert s["termination"] == s0["termination"] and s["num_iterations"] == s0["num_iterations"] == len(hist) == len(hist0)
    assert [h["accepted"] for h in hist] == [h["accepted"] for h in hist0]
    assert [h["factorization_failed"] for h in hist] == [h["factorization_failed"] for h in hist0]
    for k in KEYS:
        assert same_bits([h[k] for h in hist], [h[k] for h in hist0]), (k, [h[k] for h in hist], [h[k] for h in hist0])
    assert same_bits([s["initial_cost"], s["final_cost"]], [s0["initial_cost"], s0["final_cost"]])
    assert same_bits(x, x0), np.abs(x - x0).max()


@pytest.fixture(scope="module")
def mixed_natural(capi, ctx, mixed):
    pg = mixed.graph(capi, ctx)
    pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE)
    x, _ = pg.optimize(mixed.g["poses0"], max_solver_time_in_seconds=600.0, **ref.MIXED_SOLVE)
    pg.destroy()
    return x


@pytest.mark.parametrize("ordering", ("rcm", "given"))
def test_mixed_graph_under_an_ordering_is_the_restatement_on_the_permuted_system(capi, ctx, mixed, mixed_natural, ordering):
    g = mixed.g
    given = np.random.default_rng(8).permutation(77) if ordering == "given" else None
    code = capi.ORDER_GIVEN if ordering == "given" else capi.ORDER_RCM
    pg = mixed.graph(capi, ctx)
    pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE, code, given)
    if ordering == "rcm":
        assert "RCM" in _refused(capi, ctx, capi.ERR_INVALID, pg.order)  # made with the lists
    x, s = pg.optimize(g["poses0"], max_solver_time_in_seconds=600.0, **ref.MIXED_SOLVE)
    hist, order, stats = pg.history(), pg.order(), pg.structure()
    Hg, gg = pg.download_system()
    pg.destroy()
    keep = {}
    restated = sref.solve(g["n"], g["constant"], g["edges"], g["poses0"], ordering=code, given=given, keep=keep,
                          max_solver_time_in_seconds=600.0, **ref.MIXED_SOLVE)
    assert order.tolist() == keep["order"] and (given is None or order.tolist() == given.tolist())
    assert order.tolist() != list(range(77)) and sorted(order.tolist()) == list(range(77))
    assert stats["n_l_tiles"] == len(keep["l_tiles"]) and stats["n_h_tiles"] == len(keep["h_keys"])
    _assert_is_the_restatement(x, s, hist, restated)
    # the downloaded system is in ascending node order whatever the order in use
    P = np.repeat(4 * np.asarray(keep["order"]), 4) + np.tile(np.arange(4), 77)
    Hp = sref.to_dense(keep["H"], 308)
    H0 = np.zeros((308, 308))
    H0[np.ix_(P, P)] = Hp
    assert same_bits(Hg, H0) and same_bits(gg, keep["g"])
    dt = np.abs(x[:, :3] - mixed_natural[:, :3]).max()
    dyaw = np.rad2deg(np.abs([ref.normalize_angle(float(v)) for v in x[:, 3] - mixed_natural[:, 3]]).max())
    print(f"{ordering}: against the natural order dt {dt:.3e} m, dyaw {dyaw:.3e} deg; {stats}")
    assert dt < 1e-3 and dyaw < 0.01


# ---- 5: past the dense limit ----------------------------------------------------------------------------------------
# (the default parameter tolerance, 3e-3 of the |x| of 4200 poses tens of metres out, would stop after one accepted step)
LONG_SOLVE = dict(initial_trust_region_radius=1e8, parameter_tolerance=1e-4, max_num_iterations=6, max_solver_time_in_seconds=600.0)


def test_a_graph_past_the_dense_limit_converges_and_is_the_restatement_bit_for_bit(capi, ctx):
    """4200 nodes, nf = 16796: the dense solver refuses the graph (as before: VGX_ERR_UNSUPPORTED), the tile-sparse one
    solves it.  The restatement's solve of this graph takes about fifteen seconds on the CPU -- under the minute at which
    the comparison would be cut to two iterations -- so the whole solve is compared: two accepted steps, each with its
    re-assembly, and three factorisations.  (The factor itself is compared through vgx_block_spd_solve above: the graph
    handle has no call that returns it.)"""
    g = sref.long_graph(4200, seed=0)
    assert "free nodes" in _refused(capi, ctx, capi.ERR_UNSUPPORTED, lambda: capi.PoseGraph(ctx, 4200))
    pg = capi.PoseGraph(ctx, 4200, g["constant"], linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE)
    pg.set_edges([capi.pose_graph_edge(*e) for e in g["edges"]])
    x, s = pg.optimize(g["poses0"], **LONG_SOLVE)
    hist, stats = pg.history(), pg.structure()
    print(s, stats)
    keep = {}
    restated = sref.solve(g["n"], g["constant"], g["edges"], g["poses0"], keep=keep, **LONG_SOLVE)
    _assert_is_the_restatement(x, s, hist, restated)
    assert s["termination_type"] == capi.CONVERGENCE and s["num_successful_steps"] >= 2 and s["num_iterations"] >= 3 and s["final_cost"] < 0.1 * s["initial_cost"]
    assert stats["n_free_variables"] == 16796 and stats["n_panels"] == 263
    assert stats["n_l_tiles"] == len(keep["l_tiles"]) and stats["n_h_tiles"] == len(keep["h_keys"])
    assert stats["n_update_triples"] == len(sref.update_triples(keep["l_tiles"])) and stats["n_launches"] == sref.launches(keep["l_tiles"])
    assert stats["bytes"] >= 32768 * (stats["n_l_tiles"] + stats["n_h_tiles"]) and stats["n_l_tiles"] < 263 * 264 // 2 // 20
    # the dense H is not made past 16384 unknowns; g is still delivered
    from voxgraph_amd.capi import _ptr, f64p
    H1, gg = np.full(1, 7.0), np.zeros(16796)
    rc = ctx.lib.vgx_pose_graph_download_system(pg.h, None, _ptr(H1, f64p), _ptr(gg, f64p))
    assert rc == capi.ERR_UNSUPPORTED and H1[0] == 7.0 and "g is delivered" in ctx.lib.vgx_last_error(ctx.h).decode()
    assert same_bits(gg, keep["g"]) and same_bits(pg.download_gradient(), keep["g"])
    # covariances keep the dense factor and its limit: refused, the array untouched
    cov, pairs = np.full((1, 16), 7.0), np.array([[1, 2]], np.int32)
    rc = ctx.lib.vgx_pose_graph_covariance(pg.h, _ptr(x, f64p), 0, 1, _ptr(pairs, C.POINTER(C.c_int32)), _ptr(cov, f64p))
    assert rc == capi.ERR_UNSUPPORTED and (cov == 7.0).all() and "dense factor" in ctx.lib.vgx_last_error(ctx.h).decode()
    assert "free nodes" in _refused(capi, ctx, capi.ERR_UNSUPPORTED, lambda: pg.set_linear_solver(capi.LINEAR_SOLVER_DENSE))
    pg.destroy()


# ---- 6: switching and refusals --------------------------------------------------------------------------------------
def test_dense_sparse_dense_on_one_handle_reproduces_the_first_dense_solve_bit_for_bit(capi, ctx, ring20):
    pg = ring20.graph(capi, ctx)
    first = _solved(pg, ring20.g["poses0"])
    pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE, capi.ORDER_RCM)
    middle = _solved(pg, ring20.g["poses0"])
    cov_sparse = pg.covariance(first[0], [(1, 2), (5, 19)])               # the dense factor, whatever the setting ...
    again_sparse = _solved(pg, ring20.g["poses0"])                        # ... and the sparse lists are made again after it
    pg.set_linear_solver(capi.LINEAR_SOLVER_DENSE)
    last = _solved(pg, ring20.g["poses0"])
    cov_dense = pg.covariance(first[0], [(1, 2), (5, 19)])
    pg.destroy()
    assert same_bits(first[0], last[0]) and same_bits(first[3][0], last[3][0]) and same_bits(first[3][1], last[3][1])
    for k in KEYS:
        assert same_bits([h[k] for h in first[2]], [h[k] for h in last[2]]), k
    assert same_bits(middle[0], again_sparse[0]) and same_bits(cov_sparse, cov_dense)
    assert np.abs(middle[0] - first[0]).max() < 1e-6 and middle[1]["termination"] == first[1]["termination"]


def test_a_second_edge_list_on_a_sparse_handle_solves_as_a_fresh_graph_does(capi, ctx, mixed):
    """the chain alone after the hub: fewer tiles, and no block of the first system is left"""
    g, chain = mixed.g, mixed.edges[:79]
    kw = dict(max_num_iterations=4, exclude_registration_constraints=1)
    pg = mixed.graph(capi, ctx)
    pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE)
    pg.optimize(g["poses0"], **kw)
    tiles_first = pg.structure()["n_l_tiles"]
    pg.set_edges(chain)
    second, stats = _solved(pg, g["poses0"], **kw), pg.structure()
    pg.destroy()
    fresh = mixed.graph(capi, ctx, edges=chain)
    fresh.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE)
    third = _solved(fresh, g["poses0"], **kw)
    fresh.destroy()
    dense = mixed.graph(capi, ctx, edges=chain)
    fourth = _solved(dense, g["poses0"], **kw)
    dense.destroy()
    assert stats["n_l_tiles"] == 9 < tiles_first                           # five diagonal tiles and the four below them
    assert same_bits(second[0], third[0]) and same_bits(second[3][0], third[3][0]) and same_bits(second[3][1], third[3][1])
    _assert_same_solve(second, third)
    _assert_same_solve(second, fourth)


def test_refusals_give_a_status_and_a_text_and_change_nothing(capi, ctx, ring20):
    pg = ring20.graph(capi, ctx)
    pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE, capi.ORDER_GIVEN, np.arange(19)[::-1])
    raw = ctx.lib.vgx_pose_graph_set_linear_solver
    from voxgraph_amd.capi import _ptr, i32p
    for perm in (np.array([0] * 19, np.int32), np.arange(1, 20, dtype=np.int32), None):
        assert raw(pg.h, capi.LINEAR_SOLVER_TILE_SPARSE, capi.ORDER_GIVEN, _ptr(perm, i32p)) == capi.ERR_INVALID
        assert "permutation" in ctx.lib.vgx_last_error(ctx.h).decode()
    assert "solver" in _refused(capi, ctx, capi.ERR_INVALID, lambda: pg.set_linear_solver(2))
    assert "ordering" in _refused(capi, ctx, capi.ERR_INVALID, lambda: pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE, 3))
    assert "solver" in _refused(capi, ctx, capi.ERR_INVALID, lambda: capi.PoseGraph(ctx, 5, linear_solver=7))
    assert pg.order().tolist() == list(range(19))[::-1]                   # the refused calls changed nothing
    x, s = pg.optimize(ring20.g["poses0"])
    assert s["num_successful_steps"] >= 1 and pg.order().tolist() == list(range(19))[::-1]
    shard = capi.RegistrationBatch(ctx, ring20.cfs[:2], ring20.g["pairs"][:2], global_index=[0, 1], n_global=5)
    assert "sharded" in _refused(capi, ctx, capi.ERR_INVALID, lambda: pg.set_registration(shard))
    shard.destroy()
    x2, _ = pg.optimize(ring20.g["poses0"])
    assert same_bits(x, x2)
    pg.destroy()
