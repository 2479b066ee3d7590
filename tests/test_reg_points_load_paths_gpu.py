"""The point loads of the materialising REG pass and of the fused pass's prefetch, on every path they take.

load_tile_points (vgx_reg.hip) decides ONCE per tile where a thread's four points come from -- the reference
submap's own points and weights (all-points constraint), the batch's precomputed draw, or the in-kernel draw of the
drop-in launch -- and requests all of them before it waits for the first; the verdict of
reg_points_tile_dead_kernel reaches reg_eval_points_kernel as one bit of a 32-bit word.  None of that may change a
value: every row here is held to the project's rule, GPU f32 == f32(oracle f64) (and GPU f64 == oracle f64),
bit for bit, on
  * residual counts that leave inactive lanes (which load a clamped index) and a partial last tile in every load slot,
  * batches that alternate all-points and sampling constraints, live, fully dead and half-dead tiles, with 5 and 33
    tiles in all (33: the verdict bits run over a word boundary, a dead tile next to a live one across it),
  * every entry point that runs the body: Jacobian blocks left out, the f64 rows, the blocked layout, the drop-in call,
  * the fused pass on the same mixed batch.
Point sets have exact sizes (Submap.set_points, as tests/test_batch_sampling_gpu.py replaces points); sampling
constraints carry private engines (sampler_seed), so each is followed by its own std::mt19937 in the oracle."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from oracle import synth
from tests import helpers as H
from tests.test_ref_pin import sequential_cumsum

pytestmark = pytest.mark.gpu
F = np.float32
COUNTS = [1, 255, 256, 257, 1023, 1024, 1025, 2049]
N_POOL = 3000            # the point set the sampling constraints draw from
FAR = 60.0               # metres: a reference pose (or point) this far off maps outside every reading block box
ROWS = 1024              # rows of a materialising tile and of a block of the blocked layout
READ, NEAR_A, NEAR_B, FAR_A, FAR_B = range(5)            # pose-graph nodes


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[16, 8], ids=["vps16", "vps8"])
def world(request, capi, ctx):
    """One 3.2 m scene (sphere on a ground plane) as 16- or 8-voxel blocks; a reading submap and one submap per point
    set, all of the same scene: `sets[name]` = (gpu submap, xyz, dist, w) with exactly the named number of points,
    near the scene's surfaces (so they find correspondences) -- 'half' has its second 512-point chunk FAR away."""
    vps = request.param
    sdf = synth.sphere_ground_sdf((1.6, 1.6, 1.2), 1.0, 0.35)
    dims = (32 // vps,) * 3
    sm = synth.make_submap(sdf, 0.1, vps, (0, 0, 0), dims, trunc=0.3, esdf_max=1.0, drop_empty_blocks=True)
    bx, bd, _ = H.oracle_points(sm)
    rng = np.random.default_rng(100 + vps)

    def point_set(n):
        idx = rng.integers(0, len(bx), n)
        xyz = (bx[idx] + rng.uniform(-0.04, 0.04, (n, 3))).astype(F)
        return xyz, bd[idx].astype(F), rng.uniform(0.2, 1.0, n).astype(F)       # non-uniform weights: a real weighted draw

    sets, made = {}, []
    sizes = {str(n): n for n in COUNTS}
    sizes.update(pool=N_POOL, half=1024)
    for k, (name, n) in enumerate(sizes.items()):
        xyz, dist, w = point_set(n)
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


class Constraints:
    """A list of (point set name, reference node, residuals or None = all points) against the reading submap, as cost
    functions + a batch, and the oracle's side of it: `rows(c)` is the NEXT evaluation of constraint c (a sampling
    constraint draws on from its engine, as every evaluation of the batch and every drop-in Evaluate does)."""

    def __init__(self, capi, ctx, world, spec, seed0=1000):
        self.world, self.spec, self.ctx = world, spec, ctx
        self.cfs, self.engines, self.cums = [], {}, {}
        for c, (name, node, n) in enumerate(spec):
            g, xyz, dist, w = world["sets"][name]
            if n is None:
                cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
            else:
                ratio = F((n + 0.5) / len(w))
                cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=float(ratio),
                                          sampler_seed=seed0 + c)
                self.engines[c] = orc.Mt19937(seed0 + c)
                self.cums[c] = sequential_cumsum(w)
            cf = capi.RegistrationCostFunction(ctx, g, world["reading"], cfg)
            assert cf.num_residuals() == (len(w) if n is None else n), (c, name, n)
            self.cfs.append(cf)
        self.pairs = [(node, READ) for _, node, _ in spec]
        self.batch = capi.RegistrationBatch(ctx, self.cfs, self.pairs)
        self.ro = self.batch.row_offsets()
        self.R = self.batch.num_residuals()
        self.poses = world["poses"]

    def rows(self, c):
        name, node, n = self.spec[c]
        _, xyz, dist, w = self.world["sets"][name]
        idx = None if n is None else np.array([self.engines[c].weighted_draw(self.cums[c]) for _ in range(n)], np.int64)
        ok, r0, jo0, je0 = orc.reg_evaluate(self.world["layer"], xyz, dist, w, self.poses[node], self.poses[READ],
                                            sample_idx=idx)
        assert ok
        return r0, jo0, je0

    def all_rows(self):
        return [self.rows(c) for c in range(len(self.spec))]

    def tiles(self):
        return sum(-(-int(self.ro[c + 1] - self.ro[c]) // ROWS) for c in range(len(self.spec)))

    def evaluate(self, dtype, want_ref=True, want_read=True):
        """one evaluate_points (f32) / evaluate_points_f64 into NaN-filled arrays -> (r, jac_ref or None, jac_read or None)"""
        import torch
        tt = torch.float32 if dtype == F else torch.float64
        r = torch.full((self.R,), float("nan"), dtype=tt, device="cuda:0")
        jo = torch.full((self.R, 4), float("nan"), dtype=tt, device="cuda:0") if want_ref else None
        je = torch.full((self.R, 4), float("nan"), dtype=tt, device="cuda:0") if want_read else None
        torch.cuda.synchronize()
        f = self.batch.evaluate_points if dtype == F else self.batch.evaluate_points_f64
        status = f(self.poses, r.data_ptr(), jo.data_ptr() if want_ref else None, je.data_ptr() if want_read else None)
        self.ctx.synchronize()
        assert np.all(status == 0)
        return tuple(None if a is None else a.cpu().numpy() for a in (r, jo, je))

    def check(self, got, want, dtype, what):
        """every row of every constraint: the oracle's f64 value, rounded to the pass's type -- bit for bit"""
        r, jo, je = got
        for c, (r0, jo0, je0) in enumerate(want):
            s = slice(int(self.ro[c]), int(self.ro[c + 1]))
            assert np.array_equal(r[s], r0.astype(dtype)), (what, c, self.spec[c])
            assert jo is None or np.array_equal(jo[s], jo0.astype(dtype)), (what, "jac_ref", c, self.spec[c])
            assert je is None or np.array_equal(je[s], je0.astype(dtype)), (what, "jac_read", c, self.spec[c])

    def destroy(self):
        self.batch.destroy()
        for cf in self.cfs:
            cf.destroy()


def mixed_spec(total_tiles):
    """All-points constraints alternate with sampling ones; FAR_* reference poses make a constraint's tiles fully dead
    (an all-points constraint is culled, a sampling one is not: its rows are zeros the long way); 'half' has one live
    and one dead 512-point chunk in its one tile.  33 tiles need a second 32-bit verdict word; in constraint order the
    list puts a dead tile at index 32 behind a live one at 31, and dead and live tiles alternate all along it, so they
    meet across the word boundary in whichever order the batch launches them."""
    if total_tiles == 5:
        return [("1025", NEAR_A, None), ("pool", NEAR_B, 255), ("1024", FAR_A, None), ("pool", NEAR_A, 1)]
    assert total_tiles == 33
    return [("2049", NEAR_A, None), ("pool", NEAR_B, 1025), ("2049", FAR_A, None), ("pool", NEAR_A, 257),
            ("half", NEAR_B, None), ("1024", FAR_B, 1023), ("1024", FAR_B, None), ("pool", NEAR_A, 2049),
            ("1025", NEAR_B, None), ("pool", NEAR_B, 255), ("2049", FAR_B, None), ("pool", NEAR_A, 1),
            ("2049", NEAR_B, None), ("pool", NEAR_B, 1024), ("1024", FAR_A, None), ("pool", NEAR_A, 256),
            ("1025", NEAR_A, None), ("pool", NEAR_B, 1025), ("1024", FAR_A, None)]


def check_culling(K):
    """the geometry is what the list says: the fused pass's chunk culling reads all, none or half of an all-points
    constraint's points (a sampling constraint has nothing to cull)"""
    live = K.batch.count_live_each(K.poses)
    for c, (name, node, n) in enumerate(K.spec):
        n_all = int(K.ro[c + 1] - K.ro[c])
        if n is not None:
            assert live[c] == n_all, (c, K.spec[c])
        elif name == "half":
            assert live[c] == (0 if node in (FAR_A, FAR_B) else 512), (c, K.spec[c])
        else:
            assert live[c] == (0 if node in (FAR_A, FAR_B) else n_all), (c, K.spec[c])


@pytest.mark.parametrize("sampling", [False, True], ids=["all_points", "sampling"])
def test_residual_counts_in_every_load_slot(capi, ctx, world, sampling):
    """1 ... 2049 residuals per constraint, near (live) and far (dead, or zeros the long way): lanes past the end load
    a clamped index and write nothing, in the first, second and last load slot and in a one-row third tile; the
    sampling batch reads its precomputed draws (and the bricks the batch rule picks for an all-sampling batch)"""
    spec = []
    for n in COUNTS:
        for node in (NEAR_A, FAR_A):
            spec.append(("pool", node, n) if sampling else (str(n), node, None))
    K = Constraints(capi, ctx, world, spec)
    check_culling(K)
    for call in range(2):
        K.check(K.evaluate(F), K.all_rows(), F, ("f32", call))
    K.check(K.evaluate(np.float64), K.all_rows(), np.float64, "f64")
    K.destroy()


@pytest.mark.parametrize("total_tiles", [5, 33])
def test_mixed_batch_through_every_entry_point(capi, ctx, world, total_tiles):
    import torch
    K = Constraints(capi, ctx, world, mixed_spec(total_tiles))
    nbytes, rows, first = K.batch.blocked_layout()
    assert rows == ROWS and K.tiles() == total_tiles == int(first[-1])
    check_culling(K)
    # both Jacobian blocks, one, the other, none: four evaluations, four draws
    for want_ref, want_read in ((True, True), (False, True), (True, False), (False, False)):
        K.check(K.evaluate(F, want_ref, want_read), K.all_rows(), F, ("f32", want_ref, want_read))
    # the f64 rows: the oracle's own values; their f32 rounding is the f32 pass's row (an all-points constraint has
    # the same rows in every evaluation: compared directly; a sampling one through the oracle, draw by draw)
    got64 = K.evaluate(np.float64)
    K.check(got64, K.all_rows(), np.float64, "f64")
    got32 = K.evaluate(F)
    K.check(got32, K.all_rows(), F, "f32 after f64")
    for c, (_, _, n) in enumerate(K.spec):
        if n is None:
            s = slice(int(K.ro[c]), int(K.ro[c + 1]))
            assert all(np.array_equal(a[s].astype(F), b[s]) for a, b in zip(got64, got32)), c
    # the blocked layout: the same rows inside each constraint's tile blocks, padding untouched
    blocks = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert np.all(K.batch.evaluate_points_blocked(K.poses, blocks.data_ptr()) == 0)
    ctx.synchronize()
    B = blocks.cpu().numpy().reshape(-1, 9 * rows)
    for c, (r0, jo0, je0) in enumerate(K.all_rows()):
        n = len(r0)
        for k0 in range(0, n, rows):
            blk, m = B[int(first[c]) + k0 // rows], min(rows, n - k0)
            assert np.array_equal(blk[:m], r0[k0:k0 + m].astype(F)), (c, k0)
            assert np.array_equal(blk[rows:5 * rows].reshape(rows, 4)[:m], jo0[k0:k0 + m].astype(F)), (c, k0)
            assert np.array_equal(blk[5 * rows:].reshape(rows, 4)[:m], je0[k0:k0 + m].astype(F)), (c, k0)
            assert np.isnan(blk[m:rows]).all() and np.isnan(blk[rows:5 * rows].reshape(rows, 4)[m:]).all()
            assert np.isnan(blk[5 * rows:].reshape(rows, 4)[m:]).all()
    # the drop-in single-constraint call (f64; a sampling constraint draws IN the kernel, from the same engine): every
    # kind of constraint of the list once
    seen = set()
    for c, (name, node, n) in enumerate(K.spec):
        kind = (name == "half", node in (FAR_A, FAR_B), n is not None)
        if kind in seen:
            continue
        seen.add(kind)
        m = K.cfs[c].num_residuals()
        r1, j1, j2 = np.full(m, np.nan), np.full((m, 4), np.nan), np.full((m, 4), np.nan)
        assert K.cfs[c].Evaluate([K.poses[node], K.poses[READ]], r1, [j1, j2])
        r0, jo0, je0 = K.rows(c)
        assert np.array_equal(r1, r0) and np.array_equal(j1, jo0) and np.array_equal(j2, je0), (c, K.spec[c])
    # ... and the batch picks the streams up where the drop-in calls left them
    K.check(K.evaluate(F), K.all_rows(), F, "f32 after drop-in calls")
    K.destroy()


def test_single_constraint_device_rows_f32(capi, ctx, world):
    """the f32 instantiation of the one-constraint kernel (evaluate_device_f32): 2049 live rows, the half-dead tile
    (decided in the kernel), a culled constraint and an in-kernel draw"""
    import torch
    spec = [("2049", NEAR_A, None), ("half", NEAR_B, None), ("1025", FAR_A, None), ("pool", NEAR_A, 1025)]
    K = Constraints(capi, ctx, world, spec)
    for c, (name, node, n) in enumerate(spec):
        m = K.cfs[c].num_residuals()
        r = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda:0")
        jo = torch.full((m, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        je = torch.full((m, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert K.cfs[c].evaluate_device_f32(K.poses[node], K.poses[READ], r.data_ptr(), jo.data_ptr(), je.data_ptr())
        ctx.synchronize()
        r0, jo0, je0 = K.rows(c)
        assert np.array_equal(r.cpu().numpy(), r0.astype(F)), c
        assert np.array_equal(jo.cpu().numpy(), jo0.astype(F)) and np.array_equal(je.cpu().numpy(), je0.astype(F)), c
    K.destroy()


@pytest.mark.parametrize("total_tiles", [5, 33])
def test_fused_pass_on_the_mixed_batch(capi, ctx, world, total_tiles):
    """Two copies of the mixed batch with the same private seeds see the same first draw: the cost-only pass of the
    one returns the full pass's cost of the other BIT FOR BIT, and the 45-blocks are the sums of the materialised rows
    (the oracle's f64 rows of that draw) to within the 2e-6 of each part's largest entry that the fuzzers hold."""
    KA = Constraints(capi, ctx, world, mixed_spec(total_tiles))
    KB = Constraints(capi, ctx, world, mixed_spec(total_tiles))
    st_n, normal = KA.batch.evaluate_normal(KA.poses)
    st_c, cost = KB.batch.evaluate_cost(KB.poses)
    assert np.all(st_n == 0) and np.array_equal(st_n, st_c)
    assert np.array_equal(cost.view(np.uint64), normal[:, 0].copy().view(np.uint64)), (cost, normal[:, 0])
    for c, (r0, jo0, je0) in enumerate(KA.all_rows()):
        J = np.concatenate([jo0, je0], axis=1)
        want = np.r_[float(r0 @ r0), J.T @ r0, (J.T @ J)[np.triu_indices(8)]]
        for lo, hi in ((0, 1), (1, 9), (9, 45)):
            scale = np.abs(want[lo:hi]).max()
            err = np.abs(normal[c][lo:hi] - want[lo:hi]).max()
            print(f"tiles {total_tiles} constraint {c} {KA.spec[c]} part {lo}: scale {scale:.6e} err/scale "
                  f"{err / scale if scale > 0 else 0.0:.3e}")
            assert err <= 2e-6 * scale, (c, KA.spec[c], lo, err, scale)
    # the second evaluation of the first copy, materialised: the next draw of the same engines
    KA.check(KA.evaluate(F), KA.all_rows(), F, "f32 after the fused pass")
    KA.destroy()
    KB.destroy()
