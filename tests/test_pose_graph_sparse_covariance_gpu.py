"""The edge covariances on the tile-sparse factor (include/voxgraph_amd.h, "Pose graph: edge covariances on the
tile-sparse factor") against their sequential restatement (tests/pose_graph_sparse_covariance_ref.py), BIT FOR BIT, on
the H the call leaves behind; against vgx_block_spd_solve column by column; against the dense vgx_pose_graph_covariance
under the natural order (np.array_equal: the two may differ in the sign of a zero alone); across slab widths; past the
dense limit (4200 nodes); on a rank-deficient graph; the refusals; and what the handle does afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import pose_graph_covariance_ref as cov
from tests import pose_graph_ref as ref
from tests import pose_graph_sparse_covariance_ref as scov
from tests import pose_graph_sparse_ref as sref
from tests.test_pose_graph_covariance_cpu import untouched_node_graph
from tests.test_pose_graph_gpu import KEYS, EdgesOnly, Ring, same_bits
from tests.test_pose_graph_sparse_gpu import _blocks, block_scenes

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


def _refused(capi, code, call):
    with pytest.raises(capi.VgxError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


# ---- 1: the solve on many right-hand sides, on a caller's matrix ----------------------------------------------------
WIDTHS = (1, 31, 32, 33, 70)


def right_hand_sides(n, m, seed):
    """random, with columns of the identity (the first, a middle and the last row's) and one all-zero column where m allows"""
    B = np.random.default_rng(seed).normal(0, 1, (n, m))
    for c, row in ((m - 1, n - 1), (m // 2, n // 2), (1, 0)):
        if 0 < c < m:
            B[:, c] = np.eye(n)[:, row]
    if m >= 4:
        B[:, 3] = 0.0
    return B


@functools.lru_cache(maxsize=None)
def block_case(rows):
    """a chain with second neighbours and two closures (where the chain is long enough for them).  50 rows: the closures
    store tile (3, 0), so that (3, 1) is pure fill (with three tile rows a chain leaves no tile to fill)"""
    closures = [(i, j) for i, j in ((rows - 1, 0), (rows - 3, 1)) if 0 <= j and i - j > 2]
    m = sref.block_matrix(rows, sref.chain_pairs(rows, closures=closures), seed=rows)
    h_keys, l_tiles = sref.tile_pattern(rows, m["pairs"], list(range(rows)))
    L = scov.factor(sref.to_tiles(m["A"], [t for t in l_tiles if t in h_keys]), m["n"], l_tiles)
    return m, h_keys, l_tiles, L


@pytest.mark.parametrize("rows", (1, 15, 16, 17, 33, 50))
def test_block_spd_solve_many_is_the_restatement_and_the_single_solve_bit_for_bit(capi, ctx, rows):
    """rows 1: one tile with w = 4; 16: exactly one panel; 17: a 4-wide last panel; 33: three panels, two tiles in column 0
    (one pass of two tiles); 50: four panels, a 8-wide last one, a fill tile, three tiles in row 3 (two passes)"""
    m, h_keys, l_tiles, L = block_case(rows)
    n = m["n"]
    assert rows != 50 or set(l_tiles) - h_keys == {(3, 1)}
    for width in WIDTHS:
        B = right_hand_sides(n, width, 100 * rows + width)
        X = capi.block_spd_solve_many(ctx, rows, m["bi"], m["bj"], m["values"], B)
        X0 = scov.solve_many(L, n, l_tiles, B)
        print(f"rows {rows} m {width}: {len(l_tiles)} tiles, max |X - X0| {np.abs(X - X0).max():.3e}")
        assert same_bits(X, X0), (rows, width)
        for c in range(width):                                           # column c IS the single solve of column c
            x, _, _, _ = capi.block_spd_solve(ctx, rows, m["bi"], m["bj"], m["values"], B[:, c].copy(), want_factor=False)
            assert same_bits(X[:, c], x), (rows, width, c)
    B = right_hand_sides(n, 33, 5)                                       # X aliasing B
    X0 = scov.solve_many(L, n, l_tiles, B)
    same = capi.block_spd_solve_many(ctx, rows, m["bi"], m["bj"], m["values"], B, in_place=True)
    assert same is B and same_bits(B, X0)


def test_block_spd_solve_many_on_the_arrowhead_takes_a_last_single_tile_after_pairs_both_ways(capi, ctx):
    """block_scenes()[1156]: all 190 tiles of 19 tile rows are stored, so tile column K has 18 - K tiles below the diagonal and
    tile row K has K left of it.  An odd count above 1 is one or more passes of two tiles and then the pass of a single
    tile: columns 1, 3, .. 15 forward, rows 3, 5, .. 17 backward.  With every tile stored the history is the dense
    solver's, so X is also vgx_dense_spd_solve_many's bit for bit; m = 33: a second workgroup with one column."""
    rows, pairs = block_scenes()[1156]
    m = sref.block_matrix(rows, pairs, seed=1156)
    n = m["n"]
    h_keys, l_tiles = sref.tile_pattern(rows, m["pairs"], list(range(rows)))
    below = [len(v) - 1 for _, v in sorted(sref.columns_of(l_tiles).items())]
    assert len(l_tiles) == 190 and below == list(range(18, -1, -1)) and sum(1 for c in below if c > 1 and c % 2) == 8
    L = scov.factor(sref.to_tiles(m["A"], [t for t in l_tiles if t in h_keys]), n, l_tiles)
    B = right_hand_sides(n, 33, 1156)
    X = capi.block_spd_solve_many(ctx, rows, m["bi"], m["bj"], m["values"], B)
    X0 = scov.solve_many(L, n, l_tiles, B)
    Xd, _ = capi.dense_spd_solve_many(ctx, m["A"], B)
    print(f"arrowhead: max |X - X0| {np.abs(X - X0).max():.3e}, max |X - dense X| {np.abs(X - Xd).max():.3e}")
    assert same_bits(X, X0) and same_bits(X, Xd)
    for c in (0, 16, 32):                                                # ... and a column IS the single solve of that column
        x, _, _, _ = capi.block_spd_solve(ctx, rows, m["bi"], m["bj"], m["values"], B[:, c].copy(), want_factor=False)
        assert same_bits(X[:, c], x), c


def test_block_spd_solve_many_reports_what_is_not_positive_definite(capi, ctx):
    rows, pairs = block_scenes()[300]
    m = sref.block_matrix(rows, pairs, seed=300)
    B = right_hand_sides(300, 33, 2)
    A = m["A"].copy()
    A[70, 70] = -1e6                                                     # a pivot of the diagonal tile 1
    with pytest.raises(ref.NotPositiveDefinite):
        ref.cholesky(A)
    text = _refused(capi, capi.ERR_NOT_POSITIVE_DEFINITE, lambda: capi.block_spd_solve_many(ctx, rows, m["bi"], m["bj"], _blocks(A, m), B))
    assert "not positive definite" in text and "vgx_block_spd_solve_many" in text
    # ... and one that arrives through the fill tile (2, 1) of the arrow (tests/test_pose_graph_sparse_gpu.py: with
    # 31 < d < 32 the last node's pivot is negative only through the 16 nodes of tile 1)
    rows, pairs = block_scenes()[132]
    arrow = sref.block_matrix(rows, pairs, seed=0)

    def matrix(d):
        M = np.zeros((132, 132))
        M[:4, :4] = np.eye(4)
        for i in range(1, 33):
            M[4 * i:4 * i + 4, 4 * i:4 * i + 4] = d * np.eye(4)
            M[4 * i:4 * i + 4, :4] = M[:4, 4 * i:4 * i + 4] = np.eye(4)
        return M

    with pytest.raises(ref.NotPositiveDefinite) as bad:
        ref.cholesky(matrix(31.5))
    assert bad.value.args[0] == 128
    B = right_hand_sides(132, 8, 3)
    call = lambda: capi.block_spd_solve_many(ctx, rows, arrow["bi"], arrow["bj"], _blocks(matrix(31.5), arrow), B)  # noqa: E731
    assert "not positive definite" in _refused(capi, capi.ERR_NOT_POSITIVE_DEFINITE, call)
    good = matrix(32.5)                                                  # nothing sticks
    X = capi.block_spd_solve_many(ctx, rows, arrow["bi"], arrow["bj"], _blocks(good, arrow), B)
    Xd, _ = capi.dense_spd_solve_many(ctx, good, B)
    assert np.array_equal(X, Xd)
    for call, code, word in ((lambda: capi.block_spd_solve_many(ctx, rows, arrow["bi"], arrow["bj"], arrow["values"], np.zeros((132, 0))), capi.ERR_INVALID, "m < 1"),
                             (lambda: capi.block_spd_solve_many(ctx, 1, [0], [0], np.eye(4), np.zeros((4, 16385))), capi.ERR_UNSUPPORTED, "16384")):
        assert word in _refused(capi, code, call)


# ---- 2-4: covariance blocks -----------------------------------------------------------------------------------------
def joined_pairs(g, exclude=False):
    return ([] if exclude else [tuple(p) for p in g["pairs"]]) + [(e[0], e[1]) for e in g["edges"]]


def sparse_graph(capi, ctx, scene, ordering=None, given=None):
    pg = scene.graph(capi, ctx)
    pg.set_linear_solver(capi.LINEAR_SOLVER_TILE_SPARSE, capi.ORDER_NATURAL if ordering is None else ordering, given)
    return pg


def check_blocks(pg, g, poses, pairs, exclude=False, ordering=sref.NATURAL, given=None, max_solve_bytes=0, kept=None):
    """the call's blocks and stats against the restatement on the H the call leaves behind -> (blocks, stats, structure)"""
    blocks, stats = pg.covariance_sparse(poses, pairs, exclude_registration=exclude, max_solve_bytes=max_solve_bytes)
    if kept is None:
        Hg, _ = pg.download_system()
        nf = Hg.shape[0]
        order, place, h_keys, l_tiles = scov.structure(g["n"], g["constant"], joined_pairs(g, exclude), ordering, given)
        tiles = scov.permuted_tiles(Hg, order, h_keys)
        P = np.repeat(4 * np.asarray(order), 4) + np.tile(np.arange(4), len(order))
        assert np.array_equal(sref.to_dense(tiles, nf), Hg[np.ix_(P, P)])  # no block of H lies outside the restated tiles
        kept = dict(nf=nf, order=order, place=place, l_tiles=l_tiles, L=scov.factor(tiles, nf, l_tiles))
    blocks0 = scov.covariance_blocks(None, kept["nf"], kept["l_tiles"], kept["place"], pairs, L=kept["L"])
    print(f"{len(pairs)} pairs, {stats}: max |block| {np.abs(blocks0).max():.3e}, max difference {np.abs(blocks - blocks0).max():.3e}")
    assert blocks.shape == (len(pairs), 4, 4) and np.abs(blocks0).max() > 0
    assert same_bits(blocks, blocks0)
    assert stats == scov.expected_stats(kept["nf"], kept["l_tiles"], kept["place"], pairs, max_solve_bytes)
    assert pg.order().tolist() == list(kept["order"])
    return blocks, stats, kept


def edge_pairs(g, exclude=False):
    """every constraint in both directions, (a, a) of some nodes, a duplicate, pairs with the constant node 0"""
    joined = joined_pairs(g, exclude)
    free = [k for k in range(g["n"]) if not g["constant"][k]]
    return [p for a, b in joined for p in ((a, b), (b, a))] + [(k, k) for k in free[::7]] + [joined[0], (0, free[1]), (free[-1], 0), (0, 0)]


@pytest.fixture(scope="module")
def ring20(capi, ctx):
    r = Ring(capi, ctx, 20)
    yield r
    r.destroy()


@pytest.fixture(scope="module")
def mixed(capi):
    return EdgesOnly(capi, ref.mixed_graph(80, ref.MIXED_SEED))


@pytest.fixture(scope="module")
def chain300(capi):
    return EdgesOnly(capi, cov.chain_graph(300))


def natural_next_to_dense(capi, ctx, scene, exclude=False):
    g = scene.g
    pairs = edge_pairs(g, exclude)
    pg, twin = sparse_graph(capi, ctx, scene), scene.graph(capi, ctx)
    blocks, stats, kept = check_blocks(pg, g, g["poses0"], pairs, exclude)
    dense = twin.covariance(g["poses0"], pairs, exclude_registration=exclude)
    pg.destroy()
    twin.destroy()
    assert np.array_equal(blocks, dense)                                 # as numbers: the sign of a zero is free
    for (a, b), block in zip(pairs, blocks):                             # zeros exactly where a constant node is named
        assert (not block.any()) == bool(g["constant"][a] or g["constant"][b]), (a, b)
    return stats, kept


@pytest.mark.parametrize("exclude", (False, True))
def test_ring_of_20_in_natural_order_is_the_restatement_and_equals_the_dense_call(capi, ctx, ring20, exclude):
    stats, kept = natural_next_to_dense(capi, ctx, ring20, exclude)
    assert kept["nf"] == 76 and stats["n_columns"] == 76 and stats["n_slabs"] == 1


def test_mixed_graph_in_natural_order_is_the_restatement_and_equals_the_dense_call(capi, ctx, mixed):
    """nf = 308: five panels, constant nodes inside (0, 26, 54), the hub's long edges"""
    stats, kept = natural_next_to_dense(capi, ctx, mixed)
    assert kept["nf"] == 308 and stats["n_columns"] == 308


def test_chain_of_300_in_natural_order_is_the_restatement_and_equals_the_dense_call(capi, ctx, chain300):
    stats, kept = natural_next_to_dense(capi, ctx, chain300)
    assert kept["nf"] == 1196 and len(kept["l_tiles"]) < 19 * 20 // 2 // 2


@pytest.mark.parametrize("ordering", ("rcm", "reversed"))
@pytest.mark.parametrize("scene", ("mixed", "components"))
def test_blocks_under_an_ordering_are_the_restatement_on_the_permuted_system(capi, ctx, mixed, scene, ordering):
    """RCM is made by the call itself, before any solve.  Two disconnected components with a hub in one: RCM orders
    component by component"""
    sc = mixed if scene == "mixed" else EdgesOnly(capi, scov.two_components(50))
    g = sc.g
    nfree = g["constant"].count(0) if isinstance(g["constant"], list) else int(np.count_nonzero(np.asarray(g["constant"]) == 0))
    given = np.arange(nfree)[::-1].copy() if ordering == "reversed" else None
    code = capi.ORDER_GIVEN if ordering == "reversed" else capi.ORDER_RCM
    pg = sparse_graph(capi, ctx, sc, code, given)
    if ordering == "rcm":
        assert "RCM" in _refused(capi, capi.ERR_INVALID, pg.order)      # no lists yet
    pairs = edge_pairs(g)
    blocks, stats, kept = check_blocks(pg, g, g["poses0"], pairs, ordering=code, given=given)
    assert list(kept["order"]) != list(range(nfree))
    twin = sc.graph(capi, ctx)
    dense = twin.covariance(g["poses0"], pairs)
    twin.destroy()
    pg.destroy()
    scale = np.abs(dense).max()
    print(f"{scene} {ordering}: against the dense call max difference {np.abs(blocks - dense).max():.3e} at scale {scale:.3e}")


def test_slab_widths_change_no_bit_on_the_chain_of_300(capi, ctx, chain300):
    """every node a second node: 1196 columns, 38 chunks; S = 32 (38 slabs), S = 64 (19) and the default (one)"""
    g = chain300.g
    pairs = [(k, k) for k in range(1, 300)] + [(299, 1), (1, 299), (150, 30), (30, 150), (0, 7), (200, 0)]
    nf = 1196
    pg = sparse_graph(capi, ctx, chain300)
    first, stats1, kept = check_blocks(pg, g, g["poses0"], pairs)
    assert (stats1["n_columns"], stats1["n_slabs"], stats1["solve_bytes"]) == (1196, 1, 8 * nf * 1196)
    results = [(first, stats1)]
    for budget, S in ((8 * nf * 32, 32), (8 * nf * 64 + 100, 64), (1, 32)):
        blocks, stats, _ = check_blocks(pg, g, g["poses0"], pairs, max_solve_bytes=budget, kept=kept)
        assert stats["n_slabs"] == -(-1196 // S) and stats["n_columns"] == 1196
        assert stats["solve_bytes"] == 8 * nf * S <= max(budget, 8 * nf * 32)
        assert stats["n_launches"] == 1 + sref.launches(kept["l_tiles"]) + 4 * stats["n_slabs"]
        results.append((blocks, stats))
    for blocks, _ in results[1:]:
        assert same_bits(blocks, first)
    pg.destroy()


# ---- 5: past the dense limit ----------------------------------------------------------------------------------------
def test_a_graph_past_the_dense_limit_gives_the_restated_blocks_bit_for_bit(capi, ctx):
    """4200 nodes, nf = 16796, at the start poses, no solve.  Sixteen second nodes: the first two free nodes, the twelve
    ends of the six closures, the last two nodes -- and the far corners (1, 4199), (4199, 1), so that the last chunk's
    backward pass runs to the first panel.  One restated factorisation."""
    g = sref.long_graph(4200, seed=0)
    closures = [(e[0], e[1]) for e in g["edges"][-6:]]
    pairs = [(1, 1), (2, 1), (1, 2), (2, 2)] + [p for a, b in closures for p in ((a, b), (b, a))]
    pairs += [(4198, 4199), (4199, 4198), (4198, 4198), (4199, 4199), (1, 4199), (4199, 1), (0, 4199), (2100, 0)]
    pg = capi.PoseGraph(ctx, 4200, g["constant"], linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE)
    pg.set_edges([capi.pose_graph_edge(*e) for e in g["edges"]])
    blocks, stats = pg.covariance_sparse(g["poses0"], pairs)
    gg, structure = pg.download_gradient(), pg.structure()
    # the dense call still refuses this graph (output untouched); the sparse call goes on working after it
    out = np.full((1, 16), 7.0)
    pr = np.array([[1, 2]], np.int32)
    from voxgraph_amd.capi import _ptr, f64p, i32p
    rc = ctx.lib.vgx_pose_graph_covariance(pg.h, _ptr(np.ascontiguousarray(g["poses0"]), f64p), 0, 1, _ptr(pr, i32p), _ptr(out, f64p))
    assert rc == capi.ERR_UNSUPPORTED and (out == 7.0).all()
    again, _ = pg.covariance_sparse(g["poses0"], pairs[:6])
    pg.destroy()
    order, place, h_keys, l_tiles = scov.structure(4200, g["constant"], joined_pairs(g))
    terms = [ref.edge_terms(e, g["poses0"][e[0]], g["poses0"][e[1]]) for e in g["edges"]]
    H, g0, _, _ = sref.assemble(4200, g["constant"], g["edges"], terms, order)
    blocks0 = scov.covariance_blocks(H, 16796, l_tiles, place, pairs)
    print(f"{stats}; {structure}; max |block| {np.abs(blocks0).max():.3e}, max difference {np.abs(blocks - blocks0).max():.3e}")
    assert same_bits(gg, g0)
    assert same_bits(blocks, blocks0) and same_bits(again, blocks0[:6])
    assert not blocks[-2:].any() and all(np.abs(b).max() > 0 for b in blocks[:-2])
    assert stats == scov.expected_stats(16796, l_tiles, place, pairs)
    assert stats["n_columns"] == 64 and stats["n_slabs"] == 1 and structure["n_l_tiles"] == len(l_tiles) and structure["n_panels"] == 263


# ---- 6: rank deficiency ---------------------------------------------------------------------------------------------
def test_a_rank_deficient_graph_is_reported_and_nothing_sticks(capi, ctx):
    g = untouched_node_graph()
    full = cov.chain_graph(6, seed=1)
    pg = sparse_graph(capi, ctx, EdgesOnly(capi, g))
    text = _refused(capi, capi.ERR_NOT_POSITIVE_DEFINITE, lambda: pg.covariance_sparse(g["poses0"], [(1, 2), (4, 4)]))
    assert "rank deficient" in text and "vgx_pose_graph_covariance_sparse" in text
    pg.set_edges([capi.pose_graph_edge(*e) for e in full["edges"]])       # the node joined to the graph again
    check_blocks(pg, full, full["poses0"], [(1, 2), (4, 4), (5, 1)])
    pg.destroy()


# ---- 7: refusals ----------------------------------------------------------------------------------------------------
def test_refusals_give_a_status_and_a_text_and_leave_the_output_untouched(capi, ctx):
    g = cov.chain_graph(6, seed=1)
    scene = EdgesOnly(capi, g)
    pg = sparse_graph(capi, ctx, scene)
    lib, f64p, i32p = ctx.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    call = lib.vgx_pose_graph_covariance_sparse
    poses = np.ascontiguousarray(g["poses0"])
    pairs = np.array([[1, 2], [3, 3]], np.int32)
    out = np.full((2, 16), 7.0)
    P, Q, O = poses.ctypes.data_as(f64p), pairs.ctypes.data_as(i32p), out.ctypes.data_as(f64p)

    def refused(rc, code, text):
        assert rc == code, rc
        assert text in lib.vgx_last_error(ctx.h).decode(), lib.vgx_last_error(ctx.h).decode()
        assert (out == 7.0).all()                                         # a refused call leaves the output untouched

    assert call(None, P, 0, 2, Q, 0, O, None) == capi.ERR_INVALID
    refused(call(pg.h, None, 0, 2, Q, 0, O, None), capi.ERR_INVALID, "NULL")
    refused(call(pg.h, P, 0, 2, None, 0, O, None), capi.ERR_INVALID, "NULL")
    refused(call(pg.h, P, 0, 2, Q, 0, None, None), capi.ERR_INVALID, "NULL")
    refused(call(pg.h, P, 0, -1, Q, 0, O, None), capi.ERR_INVALID, "n_pairs < 0")
    refused(call(pg.h, P, 0, 2, Q, -1, O, None), capi.ERR_INVALID, "max_solve_bytes < 0")
    refused(call(pg.h, P, 0, (1 << 26) + 1, Q, 0, O, None), capi.ERR_UNSUPPORTED, "2^26")
    assert call(pg.h, None, 0, 0, None, 0, None, None) == capi.OK and (out == 7.0).all()
    for bad in ([[1, 6], [3, 3]], [[1, 2], [-1, 3]]):
        Qb = np.array(bad, np.int32)
        refused(call(pg.h, P, 0, 2, Qb.ctypes.data_as(i32p), 0, O, None), capi.ERR_INVALID, "out of range")
    nan = poses.copy()
    nan[4, 1] = np.nan
    refused(call(pg.h, nan.ctypes.data_as(f64p), 0, 2, Q, 0, O, None), capi.ERR_INVALID, "not finite")
    bare = capi.PoseGraph(ctx, 6, linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE)
    refused(call(bare.h, P, 0, 2, Q, 0, O, None), capi.ERR_INVALID, "without constraints")
    bare.destroy()
    dense = scene.graph(capi, ctx)                                        # the dense solver: refused, pointing to the dense call
    refused(call(dense.h, P, 0, 2, Q, 0, O, None), capi.ERR_INVALID, "vgx_pose_graph_covariance takes the dense factor")
    assert call(dense.h, None, 0, 0, None, 0, None, None) == capi.OK
    dense.destroy()
    stats = capi.PoseGraphCovarianceStats()
    assert call(pg.h, P, 0, 2, Q, 0, O, C.byref(stats)) == capi.OK and np.isfinite(out).all() and (out != 7.0).all()
    assert (stats.n_columns, stats.n_slabs) == (8, 1)
    pg.destroy()
    fixed = capi.PoseGraph(ctx, 6, [1] * 6, linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE)   # all nodes constant: zeros
    fixed.set_edges(scene.edges)
    assert not fixed.covariance_sparse(poses, pairs)[0].any()
    fixed.destroy()


# ---- 8: the handle afterwards ---------------------------------------------------------------------------------------
def _solved(pg, poses0):
    x, s = pg.optimize(poses0, max_solver_time_in_seconds=600.0, **ref.MIXED_SOLVE)
    return x, s, pg.history()


def _same_solve(a, b):
    assert same_bits(a[0], b[0]) and a[1]["termination"] == b[1]["termination"] and len(a[2]) == len(b[2]) >= 1
    for k in KEYS + ("accepted", "factorization_failed"):
        assert same_bits(np.asarray([h[k] for h in a[2]], np.float64), np.asarray([h[k] for h in b[2]], np.float64)), k


@pytest.mark.parametrize("first", ("optimize", "dense covariance"))
def test_the_handle_afterwards_solves_and_gives_dense_covariances_as_a_fresh_one_does(capi, ctx, mixed, first):
    g = mixed.g
    pairs = edge_pairs(g)[:40]
    fresh = sparse_graph(capi, ctx, mixed, capi.ORDER_RCM)
    solved0 = _solved(fresh, g["poses0"])
    fresh.destroy()
    fresh = sparse_graph(capi, ctx, mixed, capi.ORDER_RCM)
    dense0 = fresh.covariance(g["poses0"], pairs)
    fresh.destroy()
    pg = sparse_graph(capi, ctx, mixed, capi.ORDER_RCM)
    blocks, _ = pg.covariance_sparse(g["poses0"], pairs)
    Hg, gg = pg.download_system()                                        # this evaluation's H and g, in ascending node order
    H0, g0 = cov.assembled_system(g)
    assert same_bits(Hg, H0) and same_bits(gg, g0)
    if first == "optimize":
        solved = _solved(pg, g["poses0"])
        dense = pg.covariance(g["poses0"], pairs)
    else:
        dense = pg.covariance(g["poses0"], pairs)
        solved = _solved(pg, g["poses0"])
    again, _ = pg.covariance_sparse(g["poses0"], pairs)                  # ... and the sparse lists are made again after the dense call
    pg.destroy()
    _same_solve(solved, solved0)
    assert same_bits(dense, dense0) and same_bits(again, blocks)
