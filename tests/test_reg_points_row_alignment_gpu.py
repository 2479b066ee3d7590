"""The materialising REG pass at every alignment of a constraint's first row.

A constraint's rows begin at row0 = the sum of the residual counts before it, which can be anything modulo 64, and one
store instruction of a wavefront covers 64 consecutive rows.  reg_eval_points_kernel rotates the lane-to-row assignment
inside a tile by (row0 + tile.start) & 63 (tile_local in vgx_reg.hip), so that those 64 rows are a naturally aligned span
of the output arrays; the rows that wrap are taken by the lanes the tile's first span leaves without a row.  Which lane
computes which row may not change a value, and every row of a tile must still be written exactly once, dead rows
included.  ONE batch holds every case:
  * row0 % 64 takes 0, 3, 4, 15, 16, 17, 31, 32, 48 (all-points constraints of 64 ... 2049 rows, live, fully dead -- a
    far reference pose -- and half dead) and 1, 33, 63; short sampling constraints between them set the residues;
  * at s = 1, 33 and 63 a constraint sits with each of 1, 64-s-1, 64-s, 64-s+1, 1023, 1024, 1025, 1024-s, 1024-s+1 and
    2049 residuals (64-s-1 = 0 at s = 63 is no constraint and is left out): the last tile ends before, at and after the
    wrap of the rotation, in the first span and in the last; 1024-s+1 once more with a far pose (the zero path);
  * one sampling constraint of 1025 rows at s = 63 reads its precomputed draws, which are indexed through row0 too.
Every row is held to the project's rule, GPU f32 == f32(oracle f64) and GPU f64 == oracle f64, bit for bit
(tests/test_reg_points_load_paths_gpu.py, whose scene, oracle rows and Constraints this file uses), through
evaluate_points with and without each Jacobian block, evaluate_points_f64, evaluate_points_blocked and the drop-in call
on every constraint (row0 = 0: its rows are the batch's rows bit for bit).  The outputs lie GUARD rows inside larger
buffers filled with one NaN bit pattern: afterwards no row of [0, R) holds it and every guard row still does; a second
guard of 61 rows puts the arrays off every alignment but the one their element type needs.  The batch is held to the
plain launch order, where the rotation applies (asserted); a batch in the grouped launch order keeps its loads aligned
and is checked by a test of its own."""
import numpy as np
import pytest

from oracle import synth
from tests import helpers as H
from tests.test_reg_points_load_paths_gpu import (FAR, FAR_A, FAR_B, NEAR_A, NEAR_B, N_POOL, READ, ROWS, Constraints,
                                                  capi, ctx)  # noqa: F401  (capi, ctx: fixtures)

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 64
PATTERN32 = 0x7FC5A5A5                     # quiet NaNs no arithmetic produces
PATTERN64 = 0x7FF85A5A5A5A5A5A
SPECIAL = (1, 33, 63)
RESIDUES = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 48, 63)
# residue -> the all-points constraint that sits there (point set, reference node)
OTHER = {0: ("1025", NEAR_A), 3: ("half", NEAR_B), 4: ("2049", FAR_A), 15: ("1024", NEAR_A), 16: ("1023", NEAR_B),
         17: ("half", NEAR_A), 31: ("1025", FAR_B), 32: ("2049", NEAR_B), 48: ("64", NEAR_A)}


def special_counts(s):
    return sorted({1, 64 - s - 1, 64 - s, 64 - s + 1, 1023, 1024, 1025, 1024 - s, 1024 - s + 1, 2049} - {0})


def make_spec():
    """-> (spec for Constraints, {constraint: intended row0 % 64})"""
    spec, placed, row = [], {}, 0

    def put(s, item, rows):
        nonlocal row
        need = (s - row) % 64
        if need:                                             # a short sampling constraint moves the next row0 to s mod 64
            spec.append(("pool", NEAR_B if len(spec) % 2 else NEAR_A, need))
            row += need
        placed[len(spec)] = s
        spec.append(item)
        row += rows

    for s, (name, node) in sorted(OTHER.items()):
        put(s, (name, node, None), 1024 if name == "half" else int(name))
    for s in SPECIAL:
        for k, n in enumerate(special_counts(s)):
            put(s, (str(n), NEAR_B if k % 2 else NEAR_A, None), n)
        put(s, (str(1024 - s + 1), FAR_A, None), 1024 - s + 1)
    put(63, ("pool", NEAR_A, 1025), 1025)
    return spec, placed


@pytest.fixture(scope="module", params=[16, 8], ids=["vps16", "vps8"])
def world(request, capi, ctx):  # noqa: F811
    """the scene of tests/test_reg_points_load_paths_gpu.py with one point set per residual count used here"""
    vps = request.param
    sdf = synth.sphere_ground_sdf((1.6, 1.6, 1.2), 1.0, 0.35)
    sm = synth.make_submap(sdf, 0.1, vps, (0, 0, 0), (32 // vps,) * 3, trunc=0.3, esdf_max=1.0, drop_empty_blocks=True)
    bx, bd, _ = H.oracle_points(sm)
    rng = np.random.default_rng(300 + vps)
    spec, _ = make_spec()
    sizes = {name: int(name) for name, _, n in spec if n is None and name != "half"}
    sizes.update(pool=N_POOL, half=1024)
    sets, made = {}, []
    for k, (name, n) in enumerate(sizes.items()):
        idx = rng.integers(0, len(bx), n)
        xyz = (bx[idx] + rng.uniform(-0.04, 0.04, (n, 3))).astype(F)
        dist, w = bd[idx].astype(F), rng.uniform(0.2, 1.0, n).astype(F)
        if name == "half":
            xyz[512:, 0] += F(FAR)
        g = H.gpu_submap(capi, ctx, sm, k + 1)
        g.set_points(capi.POINTS_VOXELS, xyz, dist, w, capi.POINTS_KEEP_ORDER)
        assert g.num_points(capi.POINTS_VOXELS) == n
        sets[name] = (g, xyz, dist, w)
        made.append(g)
    reading = H.gpu_submap(capi, ctx, sm, 0)
    made.append(reading)
    poses = np.zeros((5, 4))
    poses[[NEAR_A, NEAR_B]] = rng.normal(0, 0.03, (2, 4))
    poses[[FAR_A, FAR_B]] = rng.normal(0, 0.03, (2, 4)) + [[FAR, 0, 0, 0], [0, -FAR, 0, 0.3]]
    yield dict(sets=sets, reading=reading, layer=H.oracle_layer(sm), poses=poses)
    for g in made:
        g.destroy()


class Aligned(Constraints):
    """Constraints whose all-points oracle rows are computed once (they are the same in every evaluation; a sampling
    constraint's follow its engine, draw by draw) and whose outputs lie inside pattern-filled buffers"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.fixed = {}

    def rows(self, c):
        if self.spec[c][2] is not None:
            return super().rows(c)
        if c not in self.fixed:
            self.fixed[c] = super().rows(c)
        return self.fixed[c]

    def evaluate(self, dtype, want_ref=True, want_read=True, guard=GUARD):
        """one evaluation into arrays that start `guard` rows inside pattern-filled buffers -> (r, jac_ref, jac_read),
        after the sentinel checks: no row of [0, R) keeps the pattern, every guard row does"""
        import torch
        it, pattern = (torch.int32, PATTERN32) if dtype == F else (torch.int64, PATTERN64)
        size = np.dtype(dtype).itemsize
        R = self.R
        bufs = [torch.full(((R + 2 * guard) * k,), pattern, dtype=it, device="cuda:0") if want else None
                for k, want in ((1, True), (4, want_ref), (4, want_read))]
        torch.cuda.synchronize()
        ptrs = [None if b is None else b.data_ptr() + guard * k * size for b, k in zip(bufs, (1, 4, 4))]
        f = self.batch.evaluate_points if dtype == F else self.batch.evaluate_points_f64
        status = f(self.poses, *ptrs)
        self.ctx.synchronize()
        assert np.all(status == 0)
        out = []
        for b, k in zip(bufs, (1, 4, 4)):
            if b is None:
                out.append(None)
                continue
            a = b.cpu().numpy().reshape(R + 2 * guard, k)
            assert (a[:guard] == pattern).all() and (a[guard + R:] == pattern).all(), ("guard rows written", k)
            body = a[guard:guard + R]
            assert not (body == pattern).any(), ("rows left unwritten", k, np.nonzero((body == pattern).any(axis=1))[0][:8])
            body = np.ascontiguousarray(body).view(dtype)
            out.append(body[:, 0] if k == 1 else body)
        return tuple(out)


@pytest.fixture(scope="module")
def K(capi, ctx, world):  # noqa: F811
    spec, placed = make_spec()
    # The rotation applies to a launch in plain order; a batch in the grouped order keeps its point loads aligned instead
    # (launch_points).  Several constraints here share a point set, so the batch would choose the grouped order: it is held
    # to the plain one with the library's switch, which a batch reads when its first evaluation makes the order.
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VGX_POINTS_TILE_ORDER", "0")
        k = Aligned(capi, ctx, world, spec, seed0=3000)
        k.check(k.evaluate(F), k.all_rows(), F, "first evaluation")
    k.placed = placed
    yield k
    k.destroy()


def test_the_batch_is_what_the_list_says(K):
    """residues, counts at the special residues, tile mix and size"""
    counts = np.diff(K.ro)
    assert K.R < 100_000
    for c, s in K.placed.items():
        assert int(K.ro[c]) % 64 == s, (c, K.spec[c])
    assert set(K.placed.values()) == set(RESIDUES)
    for s in SPECIAL:
        have = {int(counts[c]) for c, t in K.placed.items() if t == s}
        assert have >= set(special_counts(s)), (s, have)
    live = K.batch.count_live_each(K.poses)
    for c, (name, node, n) in enumerate(K.spec):
        if n is not None:
            assert live[c] == counts[c]
        elif node in (FAR_A, FAR_B):
            assert live[c] == 0, (c, K.spec[c])                       # fully dead tiles
        else:
            assert live[c] == (512 if name == "half" else counts[c]), (c, K.spec[c])   # 'half': one half-dead tile
    assert any(n is not None and int(K.ro[c]) % 64 and counts[c] > ROWS for c, (_, _, n) in enumerate(K.spec))
    assert K.batch.launch_order(points_pass=True) == 0       # the rotation is what runs


@pytest.mark.parametrize("want_ref,want_read", [(True, True), (False, True), (True, False), (False, False)],
                         ids=["both", "read_only", "ref_only", "residuals_only"])
def test_f32_rows_with_and_without_each_jacobian_block(K, want_ref, want_read):
    got = K.evaluate(F, want_ref, want_read)
    K.check(got, K.all_rows(), F, ("f32", want_ref, want_read))


def test_f32_rows_on_arrays_61_rows_off(K):
    """bases 244 B (residuals) and 976 B (Jacobians) past a 256-byte boundary: correctness does not depend on them"""
    got = K.evaluate(F, guard=61)
    K.check(got, K.all_rows(), F, "f32, guard 61")


def test_f64_rows_and_the_drop_in_call(K):
    """evaluate_points_f64 == the oracle; then the drop-in call on EVERY constraint (its own launch, row0 = 0): an
    all-points constraint's rows equal the batch's f64 rows bit for bit, a sampling constraint's (it draws on from the
    same engine, in the kernel) the oracle's next draw; the batch then picks the streams up where the calls left them"""
    got64 = K.evaluate(np.float64)
    K.check(got64, K.all_rows(), np.float64, "f64")
    got61 = K.evaluate(np.float64, guard=61)
    K.check(got61, K.all_rows(), np.float64, "f64, guard 61")
    for c, (name, node, n) in enumerate(K.spec):
        m = K.cfs[c].num_residuals()
        r1, j1, j2 = np.full(m, np.nan), np.full((m, 4), np.nan), np.full((m, 4), np.nan)
        assert K.cfs[c].Evaluate([K.poses[node], K.poses[READ]], r1, [j1, j2])
        r0, jo0, je0 = K.rows(c)
        assert np.array_equal(r1, r0) and np.array_equal(j1, jo0) and np.array_equal(j2, je0), (c, K.spec[c])
        if n is None:
            s = slice(int(K.ro[c]), int(K.ro[c + 1]))
            assert np.array_equal(r1.view(np.uint64), got64[0][s].view(np.uint64)), (c, K.spec[c])
            assert np.array_equal(j1.view(np.uint64), got64[1][s].view(np.uint64)), (c, K.spec[c])
            assert np.array_equal(j2.view(np.uint64), got64[2][s].view(np.uint64)), (c, K.spec[c])
    got32 = K.evaluate(F)
    K.check(got32, K.all_rows(), F, "f32 after the drop-in calls")


def test_blocked_layout(K):
    """the same rows inside each constraint's tile blocks (aligned whatever row0 is: no rotation); the padding of every
    last block and the guard blocks before and after keep the pattern, no row keeps it"""
    import torch
    nbytes, rows, first = K.batch.blocked_layout()
    assert rows == ROWS and K.tiles() == int(first[-1])
    words, n_blocks = 9 * rows, int(first[-1])
    buf = torch.full(((n_blocks + 2) * words,), PATTERN32, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert np.all(K.batch.evaluate_points_blocked(K.poses, buf.data_ptr() + 4 * words) == 0)
    K.ctx.synchronize()
    want = K.all_rows()
    A = buf.cpu().numpy().reshape(-1, words)
    assert (A[0] == PATTERN32).all() and (A[-1] == PATTERN32).all()
    B = A[1:-1]
    for c, (r0, jo0, je0) in enumerate(want):
        n = len(r0)
        for k0 in range(0, n, rows):
            blk, m = B[int(first[c]) + k0 // rows], min(rows, n - k0)
            parts = (blk[:rows].reshape(rows, 1), blk[rows:5 * rows].reshape(rows, 4), blk[5 * rows:].reshape(rows, 4))
            for part, ref in zip(parts, (r0[:, None], jo0, je0)):
                assert np.array_equal(part[:m].view(F), ref[k0:k0 + m].astype(F)), (c, K.spec[c], k0)
                assert not (part[:m] == PATTERN32).any() and (part[m:] == PATTERN32).all(), (c, K.spec[c], k0)


def test_a_batch_in_grouped_launch_order(capi, ctx, world):  # noqa: F811
    """Eight constraints read ONE point set (2049 points, all live) at odd row offsets: the batch launches their tiles side
    by side (launch_order 1) and does not rotate; rows, sentinels and guards are held to the same rule"""
    spec = []
    for k in range(8):
        spec += [("pool", NEAR_A, 2 * k + 1), ("2049", NEAR_B if k % 2 else NEAR_A, None)]
    G = Aligned(capi, ctx, world, spec, seed0=5000)
    assert all(int(G.ro[c]) % 64 for c in range(1, len(spec), 2))
    got = G.evaluate(F)
    G.check(got, G.all_rows(), F, "grouped, f32")
    assert G.batch.launch_order(points_pass=True) == 1
    got = G.evaluate(np.float64, guard=61)
    G.check(got, G.all_rows(), np.float64, "grouped, f64")
    G.destroy()
