"""The tile-sparse solver's host half and its restatement, without a GPU: vgx_pose_graph_tile_pattern (pure host) against
tests/pose_graph_sparse_ref.py, the restatement against the dense one (tests/pose_graph_ref.py) under np.array_equal, and
the pattern code under AddressSanitizer and UBSan in a stand-alone program (tests/cpp/tile_pattern_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pose_graph_ref as ref
from tests import pose_graph_sparse_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi
    capi.load()
    return capi


def free_pairs(g):
    pos, nfree = ref.free_positions(g["n"], g["constant"])
    pairs = [(pos[a], pos[b]) for a, b in list(g["pairs"]) + [(e[0], e[1]) for e in g["edges"]] if pos[a] >= 0 and pos[b] >= 0]
    return nfree, pairs


def pattern_scenes():
    """name -> (free nodes, pairs of free nodes)"""
    two = [(i + 1, i) for i in range(39)] + [(i + 1, i) for i in range(41, 89)] + [(88, 45), (30, 2)]     # node 40 isolated, 90 too
    return {"chain": (100, sref.chain_pairs(100, second=False)),
            "chain2_closures": (150, sref.chain_pairs(150, closures=[(140, 5), (90, 40)])),
            "mixed_hub": free_pairs(ref.mixed_graph(80, ref.MIXED_SEED)),
            "two_components_one_isolated": (91, two)}


@pytest.mark.parametrize("name", list(pattern_scenes()))
@pytest.mark.parametrize("ordering", (sref.NATURAL, sref.RCM, sref.GIVEN))
def test_tile_pattern_and_order_are_the_restatement(capi, name, ordering):
    n, pairs = pattern_scenes()[name]
    given = np.random.default_rng(3).permutation(n) if ordering == sref.GIVEN else None
    order, tiles = capi.tile_pattern(n, pairs, ordering, given)
    order0 = sref.make_order(n, pairs, ordering, given)
    h0, l0 = sref.tile_pattern(n, pairs, order0)
    assert sorted(order.tolist()) == list(range(n))
    assert order.tolist() == order0
    assert [tuple(t) for t in tiles.tolist()] == l0
    # closed under the fill rule, every diagonal tile there, and nothing but H's lower tiles and what the rule adds
    have = set(l0)
    assert all((K, K) in have for K in range((n + 15) // 16)) and all(I >= J for I, J in l0)
    for K in sorted({J for _, J in l0}):
        below = [I for I, J in l0 if J == K and I > K]
        assert all((I, J) in have for J in below for I in below if I >= J)
    assert {t for t in h0 if t[0] >= t[1]} <= have
    if name == "two_components_one_isolated" and ordering == sref.RCM:
        # the components' lowest nodes are 0, 40, 41, 90: reversed, the last component comes first
        assert order0[0] == 90 and set(order0[1:50]) == set(range(41, 90)) and order0[50] == 40 and set(order0[51:]) == set(range(40))


def test_rcm_on_a_shuffled_chain_has_no_more_tiles_than_the_chain_in_natural_order(capi):
    n = 400
    label = np.random.default_rng(1).permutation(n)
    shuffled = [(int(label[i + 1]), int(label[i])) for i in range(n - 1)]
    _, natural = capi.tile_pattern(n, sref.chain_pairs(n, second=False))
    _, as_given = capi.tile_pattern(n, shuffled)
    order, rcm = capi.tile_pattern(n, shuffled, sref.RCM)
    print(f"L tiles: the chain {len(natural)}, shuffled in natural order {len(as_given)}, shuffled under RCM {len(rcm)}")
    assert len(rcm) <= len(natural) < len(as_given)


def test_tile_pattern_refuses_malformed_input(capi):
    for n, pairs, ordering, perm in ((0, [], 0, None), (10, [(3, 10)], 0, None), (10, [(-1, 2)], 0, None), (10, [(1, 2)], 3, None),
                                     (4, [(1, 2)], sref.GIVEN, [0, 1, 1, 3]), (4, [(1, 2)], sref.GIVEN, None)):
        with pytest.raises(ValueError):
            capi.tile_pattern(n, pairs, ordering, perm)


# ---- the restatement against the dense one --------------------------------------------------------------------------
SPARSE_SCENES = {132: dict(closures=[(30, 2)]), 300: dict(closures=[(74, 3), (50, 20)]), 600: dict(closures=[(149, 10), (120, 60), (100, 35)])}


@pytest.mark.parametrize("n", sorted(SPARSE_SCENES))
def test_sparse_restatement_equals_the_dense_restatement(n):
    m = sref.block_matrix(n // 4, sref.chain_pairs(n // 4, closures=SPARSE_SCENES[n]["closures"]), seed=n)
    order = list(range(n // 4))
    h_keys, l_tiles = sref.tile_pattern(n // 4, m["pairs"], order)
    nT = (n + 63) // 64
    assert len(l_tiles) < nT * (nT + 1) // 2                         # something is skipped
    x, L = sref.spd_solve(sref.to_tiles(m["A"], [t for t in l_tiles if t in h_keys]), n, l_tiles, m["b"])
    L0 = ref.cholesky(m["A"])
    y0 = ref.forward(L0, m["b"])
    Ld = sref.to_dense(L, n)
    assert np.array_equal(Ld, L0)
    assert np.array_equal(sref.forward(L, n, l_tiles, m["b"]), y0)
    assert np.array_equal(x, ref.backward(L0, y0))
    s = np.random.default_rng(n).uniform(-1, 1, n)
    assert np.array_equal(sref.matvec(sref.to_tiles(m["A"], h_keys), n, s), ref.matvec(m["A"], s))
    print(f"n {n}: {len(l_tiles)} of {nT * (nT + 1) // 2} tiles; bit-identical too: "
          f"{np.array_equal(Ld.view(np.uint64), L0.view(np.uint64))}")


def test_sparse_restatement_with_a_planted_negative_zero_is_still_value_equal():
    n = 132
    m = sref.block_matrix(33, sref.chain_pairs(33, closures=[(30, 2)]), seed=1)
    A = m["A"].copy()
    A[70, 3] = A[3, 70] = -0.0                                       # inside the stored tile (1, 0)
    A[131, 100] = A[100, 131] = -0.0
    h_keys, l_tiles = sref.tile_pattern(33, m["pairs"], list(range(33)))
    x, L = sref.spd_solve(sref.to_tiles(A, [t for t in l_tiles if t in h_keys]), n, l_tiles, m["b"])
    x0, L0 = ref.spd_solve(A, m["b"])
    assert np.array_equal(sref.to_dense(L, n), L0) and np.array_equal(x, x0)


def test_sparse_restatement_solves_the_mixed_graph_as_the_dense_restatement_does():
    """natural order: every number of the history equal (only the sign of a zero may differ)"""
    g = ref.mixed_graph(80, ref.MIXED_SEED)
    kw = dict(ref.MIXED_SOLVE, max_num_iterations=6, max_solver_time_in_seconds=600.0)
    x, s, hist = sref.solve(g["n"], g["constant"], g["edges"], g["poses0"], **kw)
    x0, s0, hist0 = ref.solve(ref.ZeroRegistration(), g["n"], g["constant"], g["edges"], g["poses0"], **kw)
    assert np.array_equal(x, x0) and s == s0 and hist == hist0


# ---- the pattern code under the sanitizers, in a program of its own -------------------------------------------------
def test_tile_pattern_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")                                         # the compiler the library's own Makefile names
    assert cxx is not None
    exe = str(tmp_path / "tile_pattern_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "voxgraph_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tile_pattern_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "tile_pattern_check ok" in out.stdout and "ERROR" not in out.stderr
