"""The pose-graph solve on the device (include/voxgraph_amd.h, "Pose graph: the solve") against its sequential
restatement (tests/pose_graph_ref.py), BIT FOR BIT: the dense Cholesky solve at the tile-edge sizes, the assembled
system, and whole solves -- every cost, gain ratio, radius and step norm of the history, and the end poses.  Then the
solve against the harness solver over the same GPU backend (the project's end-pose bar), and the error paths.

Mutation checks (the CPU halves are in tests/test_pose_graph_cpu.py): summing a tile's products before subtracting
fails test_dense_spd_solve_is_the_restatement_bit_for_bit (n = 68, 200, 516); swapping steps 2 and 3 of the assembly
order, or dropping the transpose at (b, a), fails test_assembled_system_is_the_restatement_bit_for_bit.

Past one panel and one workgroup, each of these was built into a copy of the library (vgx_pose_graph.hip alone
changed) and the named test run against it on an MI355X, where it failed:
  pg_forward_kernel's row loop with a stride of 2048       test_dense_spd_solve_is_the_restatement_bit_for_bit[1100]
  make_lists taking a block's row from the node index      test_assembled_system_at_scale_is_the_restatement_bit_for_bit
    (only where that index is below the free-node count: the plain mutation writes past the end of H and was not run)
  normalize_angle with trunc in place of floor             test_mixed_graph_solve_is_the_restatement_bit_for_bit
  pg_matvec_kernel's guard r >= 64 in place of r >= nf     the same, and test_solve_of_a_ring_of_20_... (both cases);
    (run against these two tests only: below 64 unknowns that guard reads and writes out of bounds)
  make_lists without the memset of d_H                     test_a_second_edge_list_on_one_handle_solves_as_a_fresh_graph_does
  the gradient stop's max through std::max (drops NaNs)    test_overflowing_edge_fails_every_factorisation_and_never_stops_...
"""
import warnings

import numpy as np
import pytest

from harness import lm
from harness.backends import GpuBackend
from tests import helpers as H
from tests import pose_graph_ref as ref
from tests.test_pose_graph_cpu import SIZES, check_mixed_history, spd_cases

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


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1-3: the factorisation on its own ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_dense_spd_solve_is_the_restatement_bit_for_bit(capi, ctx, n):
    for name, (A, b) in spd_cases(n).items():
        x, L = capi.dense_spd_solve(ctx, A, b)
        x0, L0 = ref.spd_solve(A, b)
        dl, dx = np.abs(L - L0).max(), np.abs(x - x0).max()
        print(f"n {n} {name}: max |L - L0| {dl:.3e}, max |x - x0| {dx:.3e}")
        assert same_bits(L, L0), (name, n, dl)
        assert same_bits(x, x0), (name, n, dx)


def test_dense_spd_solve_reads_the_lower_triangle_only(capi, ctx):
    A, b = spd_cases(68)["integer"]
    x0, L0 = capi.dense_spd_solve(ctx, A, b)
    M = A.copy()
    M[np.triu_indices(68, 1)] = np.nan
    x, L = capi.dense_spd_solve(ctx, M, b)
    assert same_bits(x, x0) and same_bits(L, L0)


@pytest.mark.parametrize("pivot", (0, 70, 199))
@pytest.mark.parametrize("kind", ("indefinite", "nan"))
def test_dense_spd_solve_reports_what_is_not_positive_definite(capi, ctx, pivot, kind):
    A, b = spd_cases(200)["integer"]
    M = A.copy()
    M[pivot, pivot] = np.nan if kind == "nan" else -1e6 * abs(M[pivot, pivot])
    with pytest.raises(capi.VgxError) as e:
        capi.dense_spd_solve(ctx, M, b)
    assert e.value.code == capi.ERR_NOT_POSITIVE_DEFINITE and "not positive definite" in str(e.value)
    x, L = capi.dense_spd_solve(ctx, A, b)           # nothing sticks: a good matrix afterwards is still exact
    x0, L0 = ref.spd_solve(A, b)
    assert same_bits(L, L0) and same_bits(x, x0)


@pytest.mark.parametrize("pivot", (63, 64, 65))
@pytest.mark.parametrize("kind", ("inf", "nan_below"))
def test_dense_spd_solve_reports_a_bad_pivot_beside_a_panel_edge(capi, ctx, pivot, kind):
    """+inf on the diagonal; a NaN in a below-diagonal entry (p + 3, p), which reaches the diagonal at pivot p + 3 through
    the panel solve (p = 63: the entry lies in the panel below the first tile) or inside the tile"""
    A, b = spd_cases(200)["integer"]
    M = A.copy()
    if kind == "inf":
        M[pivot, pivot] = np.inf
    else:
        M[pivot + 3, pivot] = np.nan
    with pytest.raises(ref.NotPositiveDefinite):
        ref.cholesky(M)
    with pytest.raises(capi.VgxError) as e:
        capi.dense_spd_solve(ctx, M, b)
    assert e.value.code == capi.ERR_NOT_POSITIVE_DEFINITE and "not positive definite" in str(e.value)
    x, L = capi.dense_spd_solve(ctx, A, b)
    x0, L0 = ref.spd_solve(A, b)
    assert same_bits(L, L0) and same_bits(x, x0)


@pytest.mark.parametrize("p", (1, 64, 65, 199))
def test_dense_spd_solve_of_a_rank_deficient_matrix_does_what_the_restatement_does(capi, ctx, p):
    """row and column p a copy of row and column p - 1: in exact arithmetic pivot p is 0; rounded, it is zero, negative
    or a tiny positive number.  The library refuses exactly when the restatement does, and otherwise has its bits."""
    A, b = spd_cases(200)["integer"]
    M = A.copy()
    M[p, :], M[:, p] = M[p - 1, :].copy(), M[:, p - 1].copy()
    M[p, p] = M[p - 1, p - 1]
    assert np.array_equal(M, M.T) and np.array_equal(M[p], M[p - 1]) and np.linalg.matrix_rank(M) == 199
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                # a tiny pivot may overflow the restatement's later columns
        try:
            expected = ref.spd_solve(M, b)
        except ref.NotPositiveDefinite as bad:
            expected = None
            print(f"p {p}: the restatement refuses pivot {bad.args[0]}")
    if expected is None:
        with pytest.raises(capi.VgxError) as e:
            capi.dense_spd_solve(ctx, M, b)
        assert e.value.code == capi.ERR_NOT_POSITIVE_DEFINITE
    else:
        print(f"p {p}: the restatement factorises, L[p, p] = {expected[1][p, p]:.3e}")
        x, L = capi.dense_spd_solve(ctx, M, b)
        assert same_bits(L, expected[1]) and same_bits(x, expected[0])


# ---- the graphs -----------------------------------------------------------------------------------------------------
class GpuRegistration:
    """what tests/pose_graph_ref.solve asks of the registration constraints, from the same vgx_reg_batch through capi"""

    def __init__(self, capi, ctx, batch, n_nodes, pairs):
        import torch
        self.torch, self.ctx, self.batch, self.n_nodes = torch, ctx, batch, n_nodes
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        self.buf = torch.zeros(capi.fused_size(n_nodes, batch.n), dtype=torch.float64, device="cuda")
        torch.cuda.current_stream().synchronize()

    def full(self, poses):
        _, normal = self.batch.evaluate_normal(poses)
        self.batch.assemble(self.n_nodes, self.buf.data_ptr(), zero_first=True)
        self.ctx.synchronize()
        return self.buf.cpu().numpy(), normal[:, 0].copy()

    def cost(self, poses):
        return self.batch.evaluate_cost(poses)[1]


class Ring:
    def __init__(self, capi, ctx, n, pairs=None, sampling_ratio=None):
        self.g = g = ref.ring_graph(n, seed=0)
        if pairs is not None:
            g["pairs"] = pairs
        self.submaps = [H.gpu_submap(capi, ctx, sm, i) for i, sm in enumerate(ref.ring_submaps(g))]
        for s in self.submaps:
            s.extract_voxel_points()
        kw = {} if sampling_ratio is None else dict(sampling_ratio=sampling_ratio)
        cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, **kw)
        self.cfs = [capi.RegistrationCostFunction(ctx, self.submaps[a], self.submaps[b], cfg) for a, b in g["pairs"]]
        self.batch = capi.RegistrationBatch(ctx, self.cfs, g["pairs"])
        self.edges = [capi.pose_graph_edge(*e) for e in g["edges"]]
        self.registration = GpuRegistration(capi, ctx, self.batch, n, g["pairs"])

    def graph(self, capi, ctx, edges=None, constant=None):
        pg = capi.PoseGraph(ctx, self.g["n"], self.g["constant"] if constant is None else constant)
        pg.set_registration(self.batch)
        pg.set_edges(self.edges if edges is None else edges)
        return pg

    def destroy(self):
        for o in [self.batch] + self.cfs + self.submaps:
            o.destroy()


@pytest.fixture(scope="module")
def ring(capi, ctx):
    r = Ring(capi, ctx, 12)
    yield r
    r.destroy()


# ---- 4: assembly ----------------------------------------------------------------------------------------------------
def test_assembled_system_is_the_restatement_bit_for_bit(capi, ctx):
    """6 nodes, node 0 constant; two constraints on one pair in opposite directions, a pair touching the constant node,
    three edges with full sqrt-information matrices, one of them from the constant node (an absolute constraint)"""
    pairs = [(1, 2), (2, 1), (0, 3), (3, 4), (4, 5), (2, 5)]
    r = Ring(capi, ctx, 6, pairs=pairs)
    rng = np.random.default_rng(5)
    poses = r.g["poses0"]
    edges = [(1, 2, rng.normal(0, 1, 3), 0.2, rng.normal(0, 3, (4, 4))), (0, 4, rng.normal(0, 1, 3), -0.1, rng.normal(0, 3, (4, 4))),
             (5, 2, rng.normal(0, 1, 3), 0.3, np.diag([1.0, 1.0, 50.0, 50.0]))]
    pg = r.graph(capi, ctx, edges=[capi.pose_graph_edge(*e) for e in edges])
    x, s = pg.optimize(poses, max_num_iterations=0)
    assert s["termination"] == "max_iterations" and s["num_iterations"] == 0 and s["num_full_evaluations"] == 1
    assert same_bits(x, poses)
    Hg, gg = pg.download_system()
    fused, costs = r.registration.full(poses)
    terms = [ref.edge_terms(e, poses[e[0]], poses[e[1]]) for e in edges]
    H0, g0 = ref.assemble(6, r.g["constant"], pairs, fused, edges, terms)
    assert Hg.shape == (20, 20) and np.abs(H0).max() > 0
    assert same_bits(Hg, H0), np.abs(Hg - H0).max()
    assert same_bits(gg, g0), np.abs(gg - g0).max()
    assert same_bits(Hg, Hg.T)
    cost0 = 0.0
    for c in costs:
        cost0 = cost0 + float(c)
    ecost = 0.0
    for t in terms:
        ecost = ecost + t[0]
    assert s["initial_cost"] == 0.5 * (cost0 + ecost)
    # the mutations of the order contract are other bits on this very system
    assert not same_bits(Hg, ref.assemble(6, r.g["constant"], pairs, fused, edges, terms, swap_steps_2_and_3=True)[0])
    assert not same_bits(Hg, ref.assemble(6, r.g["constant"], pairs, fused, edges, terms, drop_transpose=True)[0])
    pg.destroy()
    r.destroy()


class EdgesOnly:
    """a graph of relative-pose edges alone (tests/pose_graph_ref.mixed_graph), with what _solve_both asks of a Ring"""
    registration = None

    def __init__(self, capi, g):
        self.g, self.edges = g, [capi.pose_graph_edge(*e) for e in g["edges"]]

    def graph(self, capi, ctx, edges=None):
        pg = capi.PoseGraph(ctx, self.g["n"], self.g["constant"])
        pg.set_edges(self.edges if edges is None else edges)
        return pg


@pytest.fixture(scope="module")
def mixed(capi):
    return EdgesOnly(capi, ref.mixed_graph(80, ref.MIXED_SEED))


def test_assembled_system_at_scale_is_the_restatement_bit_for_bit(capi, ctx):
    """ref.assembly_scene: 80 nodes, 0, 26 and 54 constant (nf = 308: two blocks of the gradient kernel, free positions
    i - 1, i - 2, i - 3), the hub with 35 contributions to its diagonal block, the pair (10, 11) with two edges and two
    registration constraints in opposite directions, a registration constraint and an edge from the constant node 26"""
    g, ring6, pairs, poses = ref.assembly_scene()
    submaps = [H.gpu_submap(capi, ctx, sm, i) for i, sm in enumerate(ref.ring_submaps(ring6))]
    for s in submaps:
        s.extract_voxel_points()
    cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
    cfs = [capi.RegistrationCostFunction(ctx, submaps[a], submaps[b], cfg) for a, b in ref.ASSEMBLY_SUBMAP_PAIRS]
    batch = capi.RegistrationBatch(ctx, cfs, pairs)
    pg = capi.PoseGraph(ctx, 80, g["constant"])
    pg.set_registration(batch)
    pg.set_edges([capi.pose_graph_edge(*e) for e in g["edges"]])
    x, s = pg.optimize(poses, max_num_iterations=0)
    assert s["num_iterations"] == 0 and s["num_full_evaluations"] == 1 and same_bits(x, poses)
    Hg, gg = pg.download_system()
    fused, costs = GpuRegistration(capi, ctx, batch, 80, pairs).full(poses)
    terms = [ref.edge_terms(e, poses[e[0]], poses[e[1]]) for e in g["edges"]]
    H0, g0 = ref.assemble(80, g["constant"], pairs, fused, g["edges"], terms)
    off = np.asarray(fused[1 + 20 * 80:]).reshape(-1, 4, 4)
    assert Hg.shape == (308, 308) and all(np.abs(o).max() > 0 for o in off)         # every registration pair overlaps
    assert same_bits(Hg, H0), np.abs(Hg - H0).max()
    assert same_bits(gg, g0), np.abs(gg - g0).max()
    assert same_bits(Hg, Hg.T)
    touched = np.kron(ref.touched_blocks(80, g["constant"], pairs, g["edges"]), np.ones((4, 4), bool))
    assert not Hg[~touched].any() and (~touched).sum() > 308 * 308 // 2
    assert not same_bits(Hg, ref.assemble(80, g["constant"], pairs, fused, g["edges"], terms, swap_steps_2_and_3=True)[0])
    assert not same_bits(Hg, ref.assemble(80, g["constant"], pairs, fused, g["edges"], terms, drop_transpose=True)[0])
    pg.destroy()
    for o in [batch] + cfs + submaps:
        o.destroy()


# ---- 5: the solve ---------------------------------------------------------------------------------------------------
KEYS = ("cost", "trial_cost", "gain_ratio", "radius", "step_norm")


def _solve_both(capi, ctx, ring, exclude, poses0, **kw):
    pg = ring.graph(capi, ctx)
    x, s = pg.optimize(poses0, exclude_registration_constraints=int(exclude), max_solver_time_in_seconds=600.0, **kw)
    hist = pg.history()
    pg.destroy()
    reg = ref.ZeroRegistration() if exclude else ring.registration
    x0, s0, hist0 = ref.solve(reg, ring.g["n"], ring.g["constant"], ring.g["edges"], poses0, max_solver_time_in_seconds=600.0, **kw)
    print("library", s, "\nrestatement", s0)
    assert s["termination"] == s0["termination"] and s["num_iterations"] == s0["num_iterations"] == len(hist) == len(hist0)
    assert [h["accepted"] for h in hist] == [h["accepted"] for h in hist0]
    assert [h["factorization_failed"] for h in hist] == [h["factorization_failed"] for h in hist0]
    for k in KEYS:
        assert same_bits([h[k] for h in hist], [h[k] for h in hist0]), (k, [h[k] for h in hist], [h[k] for h in hist0])
    assert same_bits([s["initial_cost"], s["final_cost"]], [s0["initial_cost"], s0["final_cost"]])
    assert same_bits(x, x0), np.abs(x - x0).max()
    assert s["num_cost_evaluations"] == sum(1 for h in hist if h["trial_cost"] != 0.0)
    assert s["num_full_evaluations"] == 1 + sum(h["accepted"] for h in hist) == 1 + s["num_successful_steps"]
    s["history"], s["restatement"] = hist, (x0, s0, hist0)
    return x, s


@pytest.mark.parametrize("exclude", (False, True))
def test_solve_is_the_restatement_bit_for_bit(capi, ctx, ring, exclude):
    x, s = _solve_both(capi, ctx, ring, exclude, ring.g["poses0"])
    assert s["termination_type"] == capi.CONVERGENCE and s["final_cost"] < s["initial_cost"] and s["num_successful_steps"] >= 1


def test_solve_with_tight_tolerances_and_a_small_radius_is_the_restatement_bit_for_bit(capi, ctx, ring):
    """more iterations and rejected steps: a start far off, a small first radius, tolerances that let the loop run on"""
    rng = np.random.default_rng(3)
    poses0 = ring.g["poses0"] + np.concatenate([rng.normal(0, 0.15, (12, 3)), rng.normal(0, 0.1, (12, 1))], 1)
    poses0[0] = ring.g["poses0"][0]
    _solve_both(capi, ctx, ring, False, poses0, parameter_tolerance=1e-7, function_tolerance=1e-12, max_num_iterations=25,
                initial_trust_region_radius=1e-2)


def test_mixed_graph_solve_is_the_restatement_bit_for_bit(capi, ctx, mixed):
    """nf = 308: five panels, so the panel and trailing kernels of the factorisation, the second block of the damping,
    gradient and matvec kernels; accepted and rejected steps; yaw errors that wrap by one and two turns"""
    g = mixed.g
    x, s = _solve_both(capi, ctx, mixed, True, g["poses0"], **ref.MIXED_SOLVE)
    _, s0, hist0 = s["restatement"]
    check_mixed_history(g, s0, hist0)                                  # ... and the comparison above was not an empty one
    assert s["num_free_nodes"] == 77 and s["termination_type"] == capi.CONVERGENCE
    assert np.abs(x[:, 3]).max() <= np.pi and np.abs(g["poses0"][:, 3]).max() > 2 * np.pi


@pytest.fixture(scope="module")
def ring20(capi, ctx):
    r = Ring(capi, ctx, 20)
    yield r
    r.destroy()


@pytest.mark.parametrize("exclude", (False, True))
def test_solve_of_a_ring_of_20_is_the_restatement_bit_for_bit(capi, ctx, ring20, exclude):
    """nf = 76: two panels, with the fused buffer in the assembly"""
    x, s = _solve_both(capi, ctx, ring20, exclude, ring20.g["poses0"])
    assert s["num_free_nodes"] == 19 and s["num_successful_steps"] >= 1
    assert s["final_cost"] < s["initial_cost"]


def test_a_second_edge_list_on_one_handle_solves_as_a_fresh_graph_does(capi, ctx, mixed):
    """set_edges with a list that touches fewer blocks (the chain alone: no hub): no block of the first system is left"""
    g = mixed.g
    chain = mixed.edges[:79]
    kw = dict(max_num_iterations=4, max_solver_time_in_seconds=600.0)
    pg = mixed.graph(capi, ctx)
    pg.optimize(g["poses0"], **kw)
    H1, _ = pg.download_system()
    pg.set_edges(chain)
    x2, s2 = pg.optimize(g["poses0"], **kw)
    hist2, (H2, g2) = pg.history(), pg.download_system()
    pg.destroy()
    fresh = mixed.graph(capi, ctx, edges=chain)
    xf, sf = fresh.optimize(g["poses0"], **kw)
    histf, (Hf, gf) = fresh.history(), fresh.download_system()
    fresh.destroy()
    only_first = np.kron(ref.touched_blocks(80, g["constant"], [], g["edges"]) & ~ref.touched_blocks(80, g["constant"], [], g["edges"][:79]),
                         np.ones((4, 4), bool))
    assert only_first.sum() >= 16 * 50 and np.count_nonzero(H1[only_first]) > only_first.sum() // 2    # the hub's blocks were there
    assert not H2[only_first].any()
    assert same_bits(H2, Hf) and same_bits(g2, gf) and same_bits(x2, xf)
    assert s2["num_iterations"] == sf["num_iterations"] >= 2 and s2["num_successful_steps"] == sf["num_successful_steps"] >= 1
    for k in KEYS:
        assert same_bits([h[k] for h in hist2], [h[k] for h in histf]), k
    assert same_bits([s2["initial_cost"], s2["final_cost"]], [sf["initial_cost"], sf["final_cost"]])


def test_overflowing_edge_fails_every_factorisation_and_never_stops_at_the_gradient(capi, ctx):
    """two nodes, node 0 constant, one edge with sqrt_information = 1e160 I and observations of +-1e200: every input is
    finite, the residual overflows, H is inf on the diagonal and every g is a NaN (0 x inf; with the matrix alone and small
    observations g would be +-inf, which no gradient stop mistakes for zero).  max |g| of a NaN gradient is not <=
    gradient_tolerance: the loop goes on to a factorisation that fails, eight times, the radius divided by 2, 4, 8, ...
    as after any bad pivot."""
    g = dict(n=2, constant=[1, 0], edges=[(0, 1, (1e200, -1e200, 1e200), 0.3, 1e160 * np.eye(4))])
    poses0 = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 0.5]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                # the restatement overflows where the library does
        terms = [ref.edge_terms(g["edges"][0], poses0[0], poses0[1])]
        H0, g0 = ref.assemble(2, g["constant"], (), None, g["edges"], terms)
        assert np.isinf(np.diag(H0)).all() and np.isnan(g0).all()
        x, s = _solve_both(capi, ctx, EdgesOnly(capi, g), True, poses0, max_num_iterations=8)
    hist = s["history"]
    assert s["termination"] == "max_iterations" and s["termination_type"] == capi.NO_CONVERGENCE and s["num_iterations"] == 8
    assert s["num_factorization_failures"] == 8 and s["num_cost_evaluations"] == 0 and s["num_full_evaluations"] == 1
    assert s["num_successful_steps"] == 0 and np.isinf(s["initial_cost"]) and np.isinf(s["final_cost"])
    assert [h["factorization_failed"] for h in hist] == [1] * 8
    assert [h["radius"] for h in hist] == [1e4, 5e3, 1250.0, 156.25, 9.765625, 0.30517578125, 0.00476837158203125, 3.725290298461914e-05]
    assert same_bits(x, poses0)


def test_two_stage_optimise(capi, ctx, ring):
    """pose_graph_interface.cpp:182-191 on one graph handle: registration excluded, then the full problem from there"""
    pg = ring.graph(capi, ctx)
    x1, s1 = pg.optimize(ring.g["poses0"], exclude_registration_constraints=1)
    x2, s2 = pg.optimize(x1)
    xa, sa = pg.optimize(ring.g["poses0"], exclude_registration_constraints=1)      # and back: the lists follow the switch
    pg.destroy()
    assert same_bits(x1, xa) and s1["final_cost"] == sa["final_cost"]
    assert s1["num_iterations"] >= 1 and s2["termination_type"] == capi.CONVERGENCE
    assert s2["final_cost"] <= s2["initial_cost"]


def test_solve_with_sampling_constraints_terminates_and_lowers_the_cost(capi, ctx):
    """sampling constraints draw anew at every evaluation: no bit comparison, termination and a cost decrease only"""
    r = Ring(capi, ctx, 12, sampling_ratio=0.5)
    pg = r.graph(capi, ctx)
    x, s = pg.optimize(r.g["poses0"])
    print(s)
    assert s["termination_type"] in (capi.CONVERGENCE, capi.NO_CONVERGENCE) and s["num_iterations"] >= 1
    assert np.isfinite(x).all() and s["final_cost"] < s["initial_cost"]
    pg.destroy()
    r.destroy()


# ---- 6: against the harness solver ----------------------------------------------------------------------------------
def test_solve_ends_where_the_harness_solver_ends(capi, ctx, ring):
    pg = ring.graph(capi, ctx)
    x, s = pg.optimize(ring.g["poses0"], max_solver_time_in_seconds=600.0)
    pg.destroy()
    prob = lm.Problem(GpuBackend(capi, ctx, ring.batch, 12), 12, ring.g["pairs"], ref.lm_edges(ring.g["edges"]))
    xh, sh = lm.solve(prob, ring.g["poses0"], max_seconds=600)
    dt = np.abs(x[:, :3] - xh[:, :3]).max()
    dyaw = np.rad2deg(np.abs(lm.normalize_angle(x[:, 3] - xh[:, 3])).max())
    print(f"library vs harness solver: dt {dt:.3e} m, dyaw {dyaw:.3e} deg; {s['termination']} after {s['num_iterations']} / "
          f"{sh['termination']} after {sh['iterations']}")
    assert s["termination"] == sh["termination"]
    assert dt < 1e-3 and dyaw < 0.01


# ---- 7: error paths -------------------------------------------------------------------------------------------------
def _refused(capi, ctx, code, call):
    with pytest.raises(capi.VgxError) as e:
        call()
    assert e.value.code == code, e.value
    assert len(ctx.lib.vgx_last_error(ctx.h).decode()) > 10
    return str(e.value)


def test_error_paths_give_a_status_and_a_text(capi, ctx, ring):
    poses = ring.g["poses0"]
    assert "empty graph" in _refused(capi, ctx, capi.ERR_INVALID, lambda: capi.PoseGraph(ctx, 0))
    bare = capi.PoseGraph(ctx, 12)
    assert "without constraints" in _refused(capi, ctx, capi.ERR_INVALID, lambda: bare.optimize(poses))
    bad = capi.pose_graph_edge(3, 12, (0, 0, 0), 0.0, np.eye(4))
    assert "out of range" in _refused(capi, ctx, capi.ERR_INVALID, lambda: bare.set_edges([bad]))
    S_bad = np.eye(4)
    S_bad[2, 1] = -np.inf
    for t_obs, yaw_obs, S in (((0.0, np.inf, 0.0), 0.0, np.eye(4)), ((0.0, 0.0, 0.0), np.nan, np.eye(4)), ((0.0, 0.0, 0.0), 0.0, S_bad)):
        edge = capi.pose_graph_edge(3, 4, t_obs, yaw_obs, S)
        assert "not finite" in _refused(capi, ctx, capi.ERR_INVALID, lambda: bare.set_edges([ring.edges[0], edge]))
    assert "without constraints" in _refused(capi, ctx, capi.ERR_INVALID, lambda: bare.optimize(poses))   # a refused list is not kept
    bare.destroy()
    assert "free nodes" in _refused(capi, ctx, capi.ERR_UNSUPPORTED, lambda: capi.PoseGraph(ctx, 4098))
    fixed = ring.graph(capi, ctx, constant=[1] * 12)               # all nodes constant: at once, zero iterations
    x, s = fixed.optimize(poses)
    assert s["num_iterations"] == 0 and s["termination"] == "no_free_nodes" and same_bits(x, poses) and fixed.history() == []
    fixed.destroy()
    nan = poses.copy()
    nan[4, 1] = np.nan
    pg = ring.graph(capi, ctx)
    assert "not finite" in _refused(capi, ctx, capi.ERR_INVALID, lambda: pg.optimize(nan))
    pg.destroy()


def test_a_destroyed_batch_is_refused_and_freed_with_the_graph(capi, ctx):
    r = Ring(capi, ctx, 3, pairs=[(0, 1), (1, 2)])
    pg = r.graph(capi, ctx, edges=r.edges[:2])
    x, s = pg.optimize(r.g["poses0"])
    assert s["num_iterations"] >= 1
    r.batch.destroy()                                              # deferred: the graph still lists it
    assert "destroyed" in _refused(capi, ctx, capi.ERR_INVALID, lambda: pg.optimize(r.g["poses0"]))
    pg.set_registration(None)                                      # the graph lets go: the batch is freed now
    x2, s2 = pg.optimize(r.g["poses0"])
    assert s2["num_iterations"] >= 1
    pg.destroy()
    for o in r.cfs + r.submaps:
        o.destroy()
