"""The edge covariances on the device (include/voxgraph_amd.h, "Pose graph: edge covariances") against their sequential
restatement (tests/pose_graph_covariance_ref.py), BIT FOR BIT: the many-right-hand-side solve at the tile-edge sizes and
around the chunk width, the covariance blocks of the ring (registration plus edges), of the mixed graph (five panels,
three constant nodes) and of a 300-node chain (the forward skip and the backward stop at both ends), a rank-deficient
graph, and the error paths.

Mutation checks (the CPU halves are in tests/test_pose_graph_covariance_cpu.py): a panel's products summed before the
subtraction, (a, b) served as the transpose of (b, a), and damping each give other bits on the mixed graph's pairs, so
test_covariance_of_the_mixed_graph_is_the_restatement_bit_for_bit fails for a library built that way."""
import functools

import numpy as np
import pytest

from tests import pose_graph_covariance_ref as cov
from tests import pose_graph_ref as ref
from tests.test_pose_graph_covariance_cpu import mutation_pairs, untouched_node_graph
from tests.test_pose_graph_cpu import spd_cases
from tests.test_pose_graph_gpu import EdgesOnly, Ring, same_bits

pytestmark = pytest.mark.gpu

CHUNK = 32          # kSolveCols of vgx_pose_graph.hip: the columns one workgroup owns
WIDTHS = (1, 4, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


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


@pytest.fixture(scope="module")
def ring(capi, ctx):
    r = Ring(capi, ctx, 12)
    yield r
    r.destroy()


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
def factor(n, name):
    A, b = spd_cases(n)[name]
    return A, ref.cholesky(A)


# ---- 1: the solve on many right-hand sides --------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 129, 200))
def test_dense_spd_solve_many_is_the_restatement_bit_for_bit(capi, ctx, n):
    for name in ("integer", "graded"):
        A, L0 = factor(n, name)
        _, L1 = capi.dense_spd_solve(ctx, A, np.zeros(n))
        for m in WIDTHS:
            B = right_hand_sides(n, m, 100 * n + m)
            X, L = capi.dense_spd_solve_many(ctx, A, B, want_factor=True)
            X0 = cov.solve_many(L0, B)
            print(f"n {n} m {m} {name}: max |X - X0| {np.abs(X - X0).max():.3e}")
            assert same_bits(X, X0), (name, n, m)
            assert same_bits(L, L0) and same_bits(L, L1), (name, n, m)
            for c in sorted({0, 1, 3, m // 2, m - 1} & set(range(m))):          # column c IS the single solve of column c
                x, _ = capi.dense_spd_solve(ctx, A, B[:, c].copy(), want_factor=False)
                assert same_bits(X[:, c], x), (name, n, m, c)


def test_dense_spd_solve_many_past_1024_rows_is_the_restatement_bit_for_bit(capi, ctx):
    """n = 1100, m = 8: 17 panels and 12 columns, nine passes of the row update"""
    A, L0 = factor(1100, "graded")
    B = right_hand_sides(1100, 8, 7)
    X, L = capi.dense_spd_solve_many(ctx, A, B, want_factor=True)
    assert same_bits(L, L0)
    assert same_bits(X, cov.solve_many(L0, B)), np.abs(X - cov.solve_many(L0, B)).max()
    x, _ = capi.dense_spd_solve(ctx, A, B[:, 5].copy(), want_factor=False)
    assert same_bits(X[:, 5], x)


@pytest.mark.parametrize("pivot,kind", ((0, "indefinite"), (70, "indefinite"), (199, "indefinite"), (64, "inf")))
def test_dense_spd_solve_many_reports_what_is_not_positive_definite(capi, ctx, pivot, kind):
    A, L0 = factor(200, "integer")
    B = right_hand_sides(200, CHUNK + 1, 11)
    M = A.copy()
    M[pivot, pivot] = np.inf if kind == "inf" else -1e6 * abs(M[pivot, pivot])
    with pytest.raises(ref.NotPositiveDefinite) as bad:
        ref.cholesky(M)
    assert bad.value.args[0] == pivot
    with pytest.raises(capi.VgxError) as e:
        capi.dense_spd_solve_many(ctx, M, B)
    assert e.value.code == capi.ERR_NOT_POSITIVE_DEFINITE and "not positive definite" in str(e.value)
    X, _ = capi.dense_spd_solve_many(ctx, A, B)                          # nothing sticks
    assert same_bits(X, cov.solve_many(L0, B))


# ---- 2: covariance blocks -------------------------------------------------------------------------------------------
def check_blocks(pg, g, poses, pairs, exclude=False, L=None):
    """the call's blocks against the restatement on the H the call leaves behind -> (blocks, H)"""
    blocks = pg.covariance(poses, pairs, exclude_registration=exclude)
    Hg, _ = pg.download_system()
    blocks0 = cov.covariance_blocks(Hg, g["n"], g["constant"], pairs, L=L)
    print(f"{len(pairs)} pairs: max |block| {np.abs(blocks0).max():.3e}, max difference {np.abs(blocks - blocks0).max():.3e}")
    assert blocks.shape == (len(pairs), 4, 4) and np.abs(blocks0).max() > 0
    assert same_bits(blocks, blocks0)
    return blocks, Hg


@pytest.mark.parametrize("exclude", (False, True))
def test_covariance_of_the_ring_is_the_restatement_bit_for_bit(capi, ctx, ring, exclude):
    g = ring.g
    pg = ring.graph(capi, ctx)
    x, s = pg.optimize(g["poses0"], exclude_registration_constraints=int(exclude))
    assert s["num_successful_steps"] >= 1
    pairs = [p for a, b in g["pairs"] for p in ((a, b), (b, a))] + [(3, 3), (7, 7), (11, 11), (5, 6), (0, 4), (9, 0)]
    blocks, Hg = check_blocks(pg, g, x, pairs, exclude)
    pg.destroy()
    # H is the restatement's assembly at those poses
    fused = None if exclude else ring.registration.full(x)[0]
    terms = [ref.edge_terms(e, x[e[0]], x[e[1]]) for e in g["edges"]]
    H0, _ = ref.assemble(g["n"], g["constant"], () if exclude else g["pairs"], fused, g["edges"], terms)
    assert Hg.shape == (44, 44) and same_bits(Hg, H0)
    k = pairs.index((5, 6))
    assert same_bits(blocks[k], blocks[pairs.index((5, 6), k + 1)])       # the duplicate
    for (a, b), block in zip(pairs, blocks):                              # zeros exactly where the constant node 0 is named
        assert (not block.any()) == (0 in (a, b)), (a, b)


def test_covariance_of_the_mixed_graph_is_the_restatement_bit_for_bit(capi, ctx):
    """nf = 308: five panels, three constant nodes; all hub pairs, the pair (10, 11) in both directions, constant nodes"""
    g = ref.mixed_graph(80, ref.MIXED_SEED)
    pairs = mutation_pairs(g)
    pg = EdgesOnly(capi, g).graph(capi, ctx)
    blocks, Hg = check_blocks(pg, g, g["poses0"], pairs)
    assert same_bits(Hg, cov.assembled_system(g)[0])                      # the system of the CPU mutation checks
    assert not blocks[-3:].any()
    x, s = pg.optimize(g["poses0"], **ref.MIXED_SOLVE)                    # the handle solves afterwards as ever
    assert s["termination_type"] == capi.CONVERGENCE
    check_blocks(pg, g, x, pairs[:8])
    pg.destroy()


def test_covariance_of_a_chain_of_300_skips_and_stops_at_both_ends(capi, ctx):
    """nf = 1196, 19 panels.  First call: ten second nodes, 40 columns, two chunks -- the first holds the first free node
    (no panel skipped) and wants row 36 (no early stop), the second starts at the 18th panel and stops there.  Second
    call: the last free node's columns wanted at the first free node's rows and the other way round."""
    g = cov.chain_graph(300)
    pg = EdgesOnly(capi, g).graph(capi, ctx)
    pairs = [(299, 1), (150, 30), (60, 60), (100, 90), (121, 120), (10, 150), (250, 200), (251, 250), (290, 280), (285, 299)]
    blocks = pg.covariance(g["poses0"], pairs)
    Hg, _ = pg.download_system()
    assert Hg.shape == (1196, 1196)
    L = ref.cholesky(Hg)
    assert same_bits(blocks, cov.covariance_blocks(Hg, 300, g["constant"], pairs, L=L))
    check_blocks(pg, g, g["poses0"], [(1, 299), (299, 1), (299, 299)], L=L)
    check_blocks(pg, g, g["poses0"], [(298, 299), (0, 7)], L=L)            # one chunk: 18 panels skipped, then one walked
    pg.destroy()


def test_a_rank_deficient_graph_is_reported_and_nothing_sticks(capi, ctx):
    g = untouched_node_graph()
    full = cov.chain_graph(6, seed=1)
    pg = EdgesOnly(capi, g).graph(capi, ctx)
    with pytest.raises(capi.VgxError) as e:
        pg.covariance(g["poses0"], [(1, 2), (4, 4)])
    assert e.value.code == capi.ERR_NOT_POSITIVE_DEFINITE and "rank deficient" in str(e.value)
    pg.set_edges([capi.pose_graph_edge(*e) for e in full["edges"]])       # the node joined to the graph again
    check_blocks(pg, full, full["poses0"], [(1, 2), (4, 4), (5, 1)])
    x, s = pg.optimize(full["poses0"])
    assert s["num_iterations"] >= 1 and s["final_cost"] <= s["initial_cost"]
    pg.destroy()


# ---- 3: error paths -------------------------------------------------------------------------------------------------
def test_error_paths_give_a_status_and_a_text(capi, ctx):
    import ctypes as C
    g = cov.chain_graph(6, seed=1)
    pg = EdgesOnly(capi, g).graph(capi, ctx)
    lib, f64p, i32p = ctx.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    poses = np.ascontiguousarray(g["poses0"])
    pairs = np.array([[1, 2], [3, 3]], np.int32)
    out = np.full((2, 16), 7.0)
    P, Q, O = poses.ctypes.data_as(f64p), pairs.ctypes.data_as(i32p), out.ctypes.data_as(f64p)

    def refused(rc, code, text):
        assert rc == code, rc
        assert text in lib.vgx_last_error(ctx.h).decode(), lib.vgx_last_error(ctx.h).decode()
        assert (out == 7.0).all()                                         # a refused call leaves the output untouched

    assert lib.vgx_pose_graph_covariance(None, P, 0, 2, Q, O) == capi.ERR_INVALID
    refused(lib.vgx_pose_graph_covariance(pg.h, None, 0, 2, Q, O), capi.ERR_INVALID, "NULL")
    refused(lib.vgx_pose_graph_covariance(pg.h, P, 0, 2, None, O), capi.ERR_INVALID, "NULL")
    refused(lib.vgx_pose_graph_covariance(pg.h, P, 0, 2, Q, None), capi.ERR_INVALID, "NULL")
    refused(lib.vgx_pose_graph_covariance(pg.h, P, 0, -1, Q, O), capi.ERR_INVALID, "n_pairs < 0")
    assert lib.vgx_pose_graph_covariance(pg.h, None, 0, 0, None, None) == capi.OK and (out == 7.0).all()
    for bad in ([[1, 6], [3, 3]], [[1, 2], [-1, 3]]):
        Qb = np.array(bad, np.int32)
        refused(lib.vgx_pose_graph_covariance(pg.h, P, 0, 2, Qb.ctypes.data_as(i32p), O), capi.ERR_INVALID, "out of range")
    nan = poses.copy()
    nan[4, 1] = np.nan
    refused(lib.vgx_pose_graph_covariance(pg.h, nan.ctypes.data_as(f64p), 0, 2, Q, O), capi.ERR_INVALID, "not finite")
    bare = capi.PoseGraph(ctx, 6)
    refused(lib.vgx_pose_graph_covariance(bare.h, P, 0, 2, Q, O), capi.ERR_INVALID, "without constraints")
    bare.destroy()
    assert lib.vgx_pose_graph_covariance(pg.h, P, 0, 2, Q, O) == capi.OK and np.isfinite(out).all() and (out != 7.0).all()
    pg.destroy()
    fixed = capi.PoseGraph(ctx, 6, [1] * 6)                               # all nodes constant: zeros
    fixed.set_edges([capi.pose_graph_edge(*e) for e in g["edges"]])
    assert not fixed.covariance(poses, pairs).any()
    fixed.destroy()
    A, _ = spd_cases(4)["integer"]
    for call, code in ((lambda: capi.dense_spd_solve_many(ctx, np.zeros((0, 0)), np.zeros((0, 3))), capi.ERR_INVALID),
                       (lambda: capi.dense_spd_solve_many(ctx, A, np.zeros((4, 0))), capi.ERR_INVALID),
                       (lambda: capi.dense_spd_solve_many(ctx, np.zeros((1, 1)), np.zeros((1, 16385))), capi.ERR_UNSUPPORTED)):
        with pytest.raises(capi.VgxError) as e:
            call()
        assert e.value.code == code and "[1, 16384]" in str(e.value)
