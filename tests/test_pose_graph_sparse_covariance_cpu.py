"""The sparse edge covariances' restatement (tests/pose_graph_sparse_covariance_ref.py) against numpy's inverse of H in
ascending node order -- under the natural order, RCM and a reversed given order, so that a mistake in the permutation
that a kernel and a restatement by one author would share shows here -- held by the rule
tests/test_pose_graph_covariance_cpu.py applies to the dense restatement (the backward-error bound of a Cholesky solve
scaled by the condition number, twice, for numpy's own error).  Then the slab arithmetic and the column lists."""
import numpy as np
import pytest

from tests import pose_graph_covariance_ref as cov
from tests import pose_graph_ref as ref
from tests import pose_graph_sparse_covariance_ref as scov
from tests import pose_graph_sparse_ref as sref
from tests.test_pose_graph_covariance_cpu import mixed_system, ring_system
from tests.test_pose_graph_cpu import gamma

LD = np.longdouble


def chain_system():
    g = scov.chain_with_closures(60)
    return g, cov.assembled_system(g)[0]


SYSTEMS = {"ring": ring_system, "mixed": mixed_system, "chain": chain_system}


def joined_pairs(g):
    return [tuple(p) for p in g["pairs"]] + [(e[0], e[1]) for e in g["edges"]]


@pytest.mark.parametrize("ordering", ("natural", "rcm", "reversed"))
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_blocks_under_an_order_are_numpys_inverse_in_node_order_within_the_bound(name, ordering):
    """Every free node as a second node.  Column c of (P H P^T)^-1, solved over the tiles, taken back to node order, next
    to column c of numpy.linalg.inv(H): |x_c - H^-1 e_c|_2 <= 2 |H^-1|_2 |d_c|_2 with d_c = gamma(3n + 1) |L| |L^T| |x_c|,
    L the computed factor of P H P^T (norms do not see a symmetric permutation).  Then every block IS that part of the
    column, at the rows of its first node."""
    g, Hs = SYSTEMS[name]()
    n, const = g["n"], g["constant"]
    pos, nfree = ref.free_positions(n, const)
    nf = 4 * nfree
    code = dict(natural=sref.NATURAL, rcm=sref.RCM, reversed=sref.GIVEN)[ordering]
    given = list(range(nfree))[::-1] if ordering == "reversed" else None
    order, place, h_keys, l_tiles = scov.structure(n, const, joined_pairs(g), code, given)
    assert sorted(order) == list(range(nfree)) and (ordering == "natural") == (list(order) == list(range(nfree)))
    free = [k for k in range(n) if pos[k] >= 0]
    firsts = free[:5] + free[-5:]
    pairs = [(a, b) for b in free for a in firsts] + [(free[3], free[3]), (0, free[2]), (free[2], 0)]
    L = scov.factor(scov.permuted_tiles(Hs, order, h_keys), nf, l_tiles)
    blocks, X, col = scov.covariance_blocks(None, nf, l_tiles, place, pairs, L=L, want_columns=True)
    assert X.shape == (nf, nf) and not blocks[-2:].any()                # node 0 is constant in all three
    # the bound, in the permuted space
    Ld = np.abs(sref.to_dense(L, nf)).astype(LD)
    bound = (gamma(3 * nf + 1) * (Ld @ (Ld.T @ np.abs(X.astype(LD))))).astype(np.float64)
    s = np.linalg.svd(Hs, compute_uv=False)
    allowed = 2.0 / s[-1] * np.linalg.norm(bound, axis=0)
    inverse = np.linalg.inv(Hs)
    worst = 0.0
    for b in free:                                                      # columns back to node order
        for k in range(4):
            c = col[place[b]] + k
            x_node = sref.unpermuted(X[:, c], order)
            off = np.linalg.norm(x_node - inverse[:, 4 * pos[b] + k])
            worst = max(worst, off / allowed[c])
            assert off <= allowed[c], (name, ordering, b, k, off, allowed[c])
    print(f"{name} {ordering}: nf {nf}, cond {s[0] / s[-1]:.2e}, {len(l_tiles)} tiles, max |x_c - numpy's| / allowed {worst:.3e}")
    for p, (a, b) in enumerate(pairs[:-2]):
        want = inverse[4 * pos[a]:4 * pos[a] + 4, 4 * pos[b]:4 * pos[b] + 4]
        assert np.array_equal(blocks[p], X[4 * place[a]:4 * place[a] + 4, col[place[b]]:col[place[b]] + 4])
        assert np.abs(blocks[p] - want).max() <= allowed[col[place[b]]:col[place[b]] + 4].max(), (name, ordering, a, b)


def test_many_right_hand_sides_are_forward_and_backward_of_every_column():
    m = sref.block_matrix(33, [(i, 0) for i in range(1, 33)] + [(20, 19)], seed=3)      # the arrow: tile (2, 1) is pure fill
    n = m["n"]
    h_keys, l_tiles = sref.tile_pattern(33, m["pairs"], list(range(33)))
    assert set(l_tiles) - h_keys                                         # fill tiles take part
    L = scov.factor(sref.to_tiles(m["A"], [t for t in l_tiles if t in h_keys]), n, l_tiles)
    B = np.random.default_rng(1).normal(0, 1, (n, 7))
    B[:, 2] = 0.0
    B[:, 5] = np.eye(n)[:, 70]
    X = scov.solve_many(L, n, l_tiles, B)
    for c in range(7):
        x = sref.backward(L, n, l_tiles, sref.forward(L, n, l_tiles, B[:, c]))
        assert np.array_equal(X[:, c].view(np.uint64), x.view(np.uint64)), c
    assert not X[:, 2].any() and not np.signbit(X[:, 2]).any()
    np.testing.assert_allclose(m["A"] @ X, B, rtol=0, atol=1e-12)


def test_under_the_natural_order_the_blocks_equal_the_dense_restatements_as_numbers():
    g, Hs = mixed_system()
    order, place, h_keys, l_tiles = scov.structure(g["n"], g["constant"], joined_pairs(g))
    pairs = [(e[0], e[1]) for e in g["edges"]][:60] + [(10, 11), (11, 10), (0, 5), (54, 54), (40, 40)]
    sparse = scov.covariance_blocks(scov.permuted_tiles(Hs, order, h_keys), 308, l_tiles, place, pairs)
    dense = cov.covariance_blocks(Hs, g["n"], g["constant"], pairs)
    assert np.array_equal(sparse, dense) and np.abs(sparse).max() > 0


def test_slab_arithmetic():
    nf = 1196
    assert scov.slab_width(nf, 1196, 8 * nf * 32) == 32
    assert scov.slab_width(nf, 1196, 8 * nf * 64 - 1) == 32             # 8 nf S <= the budget
    assert scov.slab_width(nf, 1196, 8 * nf * 64) == 64
    assert scov.slab_width(nf, 1196, 1) == 32                            # 32 at the least, whatever the budget
    assert scov.slab_width(nf, 1196) == 1216                             # the default holds them all: the columns rounded up
    assert scov.slab_width(nf, 40) == 64 and scov.slab_width(nf, 0) == 32
    assert scov.slab_width(16796, 16796) == 7968                         # 4200 nodes, every one asked for: 1 GiB / (8 nf)
    assert 8 * 16796 * 7968 <= 1 << 30 < 8 * 16796 * (7968 + 32) and -(-16796 // 7968) == 3
    # pairs per slab: 20 free nodes (node 0 constant), seconds 3, 5 .. 19 -> 36 columns, S = 32: eight nodes and one
    place = [-1] + list(range(20))
    pairs = [(1, 5), (2, 3)] + [(k, k) for k in range(6, 20, 2)] + [(7, 19), (0, 4), (4, 0), (9, 5), (19, 18)]
    seconds, col, unit_rows, chunks = scov.column_lists(place, pairs)
    assert seconds == [2, 4, 5, 7, 9, 11, 13, 15, 17, 18] and len(unit_rows) == 40
    per_slab = scov.slab_pairs(place, pairs, col, 32)
    assert [len(s) for s in per_slab] == [9, 3] and per_slab[1] == [8, 9, 13] and sorted(per_slab[0] + per_slab[1]) == [p for p in range(14) if p not in (10, 11)]
    stats = scov.expected_stats(80, [(0, 0), (1, 0), (1, 1)], place, pairs, 8 * 80 * 32)
    assert stats == dict(n_columns=40, n_slabs=2, n_launches=1 + 4 + 8, solve_bytes=8 * 80 * 32)


def test_column_and_lowest_row_lists():
    """a reversed order over 12 nodes, node 0 constant: position = 10 - (free index)"""
    order = list(range(11))[::-1]
    place = scov.positions(12, [1] + [0] * 11, order)
    assert place == [-1] + list(range(10, -1, -1))
    pairs = [(1, 11), (5, 11), (11, 1), (3, 3), (0, 7), (7, 0), (2, 3), (3, 3)]
    seconds, col, unit_rows, chunks = scov.column_lists(place, pairs)
    assert seconds == [0, 8, 10] and col == {0: 0, 8: 4, 10: 8}          # nodes 11, 3, 1 by ascending POSITION
    assert unit_rows == [0, 1, 2, 3, 32, 33, 34, 35, 40, 41, 42, 43]
    assert chunks == [(0, 0)]                                            # (11, 1) wants row 0 of node 1's columns
    seconds, col, unit_rows, chunks = scov.column_lists(place, [(5, 3), (2, 3), (4, 1)])
    assert seconds == [8, 10] and chunks == [(32, 24)]                   # first 1 at row 4 * 8; lowest row: node 5 at 4 * 6
    many = [(k, k) for k in range(1, 12)] + [(11, 1)]
    seconds, col, unit_rows, chunks = scov.column_lists(place, many)
    assert len(unit_rows) == 44 and chunks == [(0, 0), (32, 0)]          # the second chunk: nodes 3, 2, 1; (11, 1) wants row 0
    assert scov.column_lists(place, many[:-1])[3] == [(0, 0), (32, 32)]
