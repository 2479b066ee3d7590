"""vgx_ctx_set_brick_layout: the sampling grids of a context's submaps as apron bricks (default) or quad
bricks (a 2x2x2 neighbourhood in 32 contiguous bytes, for sampling sessions).  The layout is a memory
arrangement only: every REG kernel must return bit for bit the same results on both, and those are the
oracle's / the reference source's (registration_cost_function.cpp:113-291)."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from oracle import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi
    return capi


def _world(capi, layout, asymmetric=True, sampling_bricks=None):
    ctx = capi.Context(0)
    ctx.set_brick_layout(layout)
    if sampling_bricks is not None:
        ctx.set_sampling_bricks(sampling_bricks)
    ref, read = synth.config1_pair(asymmetric=asymmetric)
    subs = [H.gpu_submap(capi, ctx, sm, k) for k, sm in enumerate((ref, read))]
    for g in subs:
        g.extract_voxel_points(1.0, 0.3, True)
    return ctx, (ref, read), subs


def test_every_kernel_gives_the_same_bits_on_both_layouts(capi):
    import torch
    poses = np.array([[0.02, -0.01, 0.03, 0.01], [0.31, -0.2, 0.08, 0.12]])
    out = {}
    # three set-ups: apron bricks with quad bricks made on demand for all-sampling batches (the default), quad
    # bricks throughout, apron bricks throughout (VGX_SAMPLING_BRICKS_SAME)
    setups = (("default", capi.BRICKS_APRON, None), ("quad", capi.BRICKS_QUAD, None),
              ("apron_only", capi.BRICKS_APRON, capi.SAMPLING_BRICKS_SAME))
    for name, layout, sampling_bricks in setups:
        ctx, (ref, read), subs = _world(capi, layout, sampling_bricks=sampling_bricks)
        res = {}
        for use_esdf in (1, 0):
            cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, use_esdf_distance=use_esdf,
                                      no_correspondence_cost=0.25)
            cf = capi.RegistrationCostFunction(ctx, subs[0], subs[1], cfg)
            n = cf.num_residuals()
            r, jo, je = np.zeros(n), np.zeros((n, 4)), np.zeros((n, 4))
            assert cf.Evaluate([poses[0], poses[1]], r, [jo, je])            # drop-in f64 kernel
            res[("evaluate", use_esdf)] = (r.copy(), jo.copy(), je.copy())
            cf.destroy()
        # batched: materialising f32 pass + fused pass, all points and sampled
        for ratio in (-1.0, 0.3):
            cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=ratio)
            cfs = [capi.RegistrationCostFunction(ctx, subs[a], subs[b], cfg) for a, b in ((0, 1), (1, 0), (0, 0))]
            batch = capi.RegistrationBatch(ctx, cfs, [(0, 1), (1, 0), (0, 0)])
            # which bricks the batch reads: quad on a quad context, and by default where every constraint samples
            want_quad = name == "quad" or (name == "default" and ratio != -1.0)
            assert batch.brick_layout() == (capi.BRICKS_QUAD if want_quad else capi.BRICKS_APRON), (name, ratio)
            R = batch.num_residuals()
            tr = torch.full((R,), float("nan"), dtype=torch.float32, device="cuda:0")
            tjo = torch.full((R, 4), float("nan"), dtype=torch.float32, device="cuda:0")
            tje = torch.full((R, 4), float("nan"), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            assert np.all(batch.evaluate_points(poses, tr.data_ptr(), tjo.data_ptr(), tje.data_ptr()) == 0)
            ctx.synchronize()
            status, normal = batch.evaluate_normal(poses)
            res[("batch", ratio)] = (tr.cpu().numpy(), tjo.cpu().numpy(), tje.cpu().numpy(), normal.copy())
            batch.destroy()
            for cf in cfs:
                cf.destroy()
        if name == "default":
            # a batch that mixes sampling and all-points constraints keeps the apron bricks
            cfg_all = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
            cfg_smp = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=0.3, sampler_seed=5)
            mixed = [capi.RegistrationCostFunction(ctx, subs[0], subs[1], cfg_all),
                     capi.RegistrationCostFunction(ctx, subs[1], subs[0], cfg_smp)]
            mb = capi.RegistrationBatch(ctx, mixed, [(0, 1), (1, 0)])
            assert mb.brick_layout() == capi.BRICKS_APRON
            mb.destroy()
            for cf in mixed:
                cf.destroy()
        out[name] = res
        if name == "default":
            # ... and they are the oracle's (all points, ESDF distance, no_correspondence_cost 0.25)
            layer = H.oracle_layer(read)
            xyz, dist, w = H.oracle_points(ref)
            ok, r0, jo0, je0 = orc.reg_evaluate(layer, xyz, dist, w, poses[0], poses[1], no_correspondence_cost=0.25)
            r, jo, je = res[("evaluate", 1)]
            assert ok and np.array_equal(r, r0) and np.array_equal(jo, jo0) and np.array_equal(je, je0)
            assert int((np.abs(jo0).sum(1) > 0).sum()) > 1000
        for g in subs:
            g.destroy()
        ctx.close()
    a = out["default"]
    for other in ("quad", "apron_only"):
        for key in a:
            for x, y in zip(a[key], out[other][key]):
                assert np.array_equal(x, y, equal_nan=True), (other, key)


def test_vps8_grids_on_both_layouts(capi):
    sdf = synth.sphere_ground_sdf((1.6, 1.6, 1.2), 1.0, 0.35)
    sm = synth.make_submap(sdf, 0.1, 8, (0, 0, 0), (4, 4, 3), trunc=0.3, esdf_max=1.0, drop_empty_blocks=True)
    poses = np.array([[0.0, 0.0, 0.0, 0.0], [0.13, -0.07, 0.04, 0.05]])
    layer = H.oracle_layer(sm)
    xyz, dist, w = H.oracle_points(sm)
    got, part = [], []
    for layout in (capi.BRICKS_APRON, capi.BRICKS_QUAD):
        ctx = capi.Context(0)
        ctx.set_brick_layout(layout)
        g = H.gpu_submap(capi, ctx, sm, 0)
        n = g.extract_voxel_points(1.0, 0.3, True)
        cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
        r, jo, je = np.zeros(n), np.zeros((n, 4)), np.zeros((n, 4))
        assert cf.Evaluate([poses[0], poses[1]], r, [jo, je])
        batch = capi.RegistrationBatch(ctx, [cf], [(0, 1)])
        _, normal = batch.evaluate_normal(poses)
        got.append((r, jo, je, normal.copy()))
        for o in (batch, cf):
            o.destroy()
        part.append(_vps8_partial_tile_entry_points(capi, ctx, g, (xyz, dist, w), poses))
        g.destroy()
        ctx.close()
    ok, r0, jo0, je0 = orc.reg_evaluate(layer, xyz, dist, w, poses[0], poses[1])
    assert ok and np.array_equal(got[0][0], r0) and np.array_equal(got[0][1], jo0) and np.array_equal(got[0][2], je0)
    for x, y in zip(got[0], got[1]):
        assert np.array_equal(x, y)
    # the partial-tile rows are the oracle's on the cropped arrays, and every entry point's output is the same on both layouts
    m = len(part[0]["rows"][0])
    ok, r0, jo0, je0 = orc.reg_evaluate(layer, xyz[:m], dist[:m], w[:m], poses[0], poses[1])
    assert ok and all(np.array_equal(x, y) for x, y in zip(part[0]["rows"], (r0, jo0, je0)))
    assert int((np.abs(jo0).sum(1) > 0).sum()) > 1000
    assert part[0].keys() == part[1].keys()
    for key in part[0]:
        for x, y in zip(part[0][key], part[1][key]):
            assert np.array_equal(x, y, equal_nan=True), key


def _vps8_partial_tile_entry_points(capi, ctx, g, points, poses):
    """The vps-8 arms of the batched entry points on a point set that ends in a partial tile and a partial chunk: the
    identities the suite asserts between them at vps 16 (tests/test_reg_gpu.py), all bit for bit.  -> what each wrote"""
    import torch
    xyz, dist, w = points
    n = 11781                                             # 11 tiles of 1024 + 517 points, 23 chunks of 512 + 5 points
    assert len(w) >= n and n % 1024 != 0 and n % 512 != 0
    g.set_points(capi.POINTS_VOXELS, xyz[:n], dist[:n], w[:n], capi.POINTS_KEEP_ORDER)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    assert cf.num_residuals() == n
    r, jo, je = np.zeros(n), np.zeros((n, 4)), np.zeros((n, 4))
    assert cf.Evaluate([poses[0], poses[1]], r, [jo, je])                    # drop-in f64 rows
    batch = capi.RegistrationBatch(ctx, [cf], [(0, 1)])
    assert batch.num_residuals() == n

    def nan_rows(dtype):
        return [torch.full(shape, float("nan"), dtype=dtype, device="cuda:0") for shape in ((n,), (n, 4), (n, 4))]

    def host(bufs):
        ctx.synchronize()
        return tuple(t.cpu().numpy() for t in bufs)

    # f64 rows into the caller's arrays and into the batch's own: the drop-in Evaluate's
    d64 = nan_rows(torch.float64)
    torch.cuda.synchronize()
    assert np.all(batch.evaluate_points_f64(poses, *(t.data_ptr() for t in d64)) == 0)
    p64 = host(d64)
    assert all(np.array_equal(x, y) for x, y in zip(p64, (r, jo, je)))
    assert np.all(batch.evaluate_rows_f64(poses) == 0)
    rows = batch.fetch_rows_f64(0, n)
    assert all(np.array_equal(x, y) for x, y in zip(rows, (r, jo, je)))
    # f32 rows: the single-constraint device pass's, and the f64 rows' rounding
    d32, s32 = nan_rows(torch.float32), nan_rows(torch.float32)
    torch.cuda.synchronize()
    assert np.all(batch.evaluate_points(poses, *(t.data_ptr() for t in d32)) == 0)
    assert cf.evaluate_device_f32(poses[0], poses[1], *(t.data_ptr() for t in s32))
    p32, single32 = host(d32), host(s32)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(p32, single32))
    assert all(np.array_equal(x.view(np.uint32), y.astype(np.float32).view(np.uint32)) for x, y in zip(p32, (r, jo, je)))
    # blocked rows, re-based with blocked_layout(): the same f32 rows, the last block's padding untouched
    nbytes, per, first = batch.blocked_layout()
    assert per == 1024 and int(first[1]) == -(-n // per) and nbytes == int(first[1]) * per * 36
    blocks = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert np.all(batch.evaluate_points_blocked(poses, blocks.data_ptr()) == 0)
    (B,) = host([blocks])
    B = B.reshape(-1, 9 * per)
    for k0 in range(0, n, per):
        blk, k = B[int(first[0]) + k0 // per], min(per, n - k0)
        s = slice(k0, k0 + k)
        assert np.array_equal(blk[:k].view(np.uint32), p32[0][s].view(np.uint32))
        assert np.array_equal(blk[per:5 * per].reshape(per, 4)[:k].view(np.uint32), p32[1][s].view(np.uint32))
        assert np.array_equal(blk[5 * per:].reshape(per, 4)[:k].view(np.uint32), p32[2][s].view(np.uint32))
        assert np.isnan(blk[k:per]).all() and np.isnan(blk[per:5 * per].reshape(per, 4)[k:]).all()
        assert np.isnan(blk[5 * per:].reshape(per, 4)[k:]).all()
    # the cost-only fused pass: element 0 of the full pass's 45-block (vgx_reg_batch_evaluate_cost)
    st_n, normal = batch.evaluate_normal(poses)
    st_c, cost = batch.evaluate_cost(poses)
    assert np.array_equal(st_n, st_c) and np.array_equal(cost.view(np.uint64), normal[:, 0].copy().view(np.uint64)) and cost[0] > 0
    for o in (batch, cf):
        o.destroy()
    return dict(rows=(r, jo, je), points_f64=p64, fetched=rows, points=p32, single=single32, blocked=(B,),
                normal=(normal.copy(),), cost=(cost.copy(),))


def test_a_batch_refuses_submaps_of_different_layouts(capi):
    ctx = capi.Context(0)
    ref, read = synth.config1_pair()
    g0 = H.gpu_submap(capi, ctx, ref, 0)
    ctx.set_brick_layout(capi.BRICKS_QUAD)
    g1 = H.gpu_submap(capi, ctx, read, 1)
    for g in (g0, g1):
        g.extract_voxel_points(1.0, 0.3, True)
    cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS)
    cfs = [capi.RegistrationCostFunction(ctx, g0, g1, cfg), capi.RegistrationCostFunction(ctx, g1, g0, cfg)]
    with pytest.raises(capi.VgxError):
        capi.RegistrationBatch(ctx, cfs, [(0, 1), (1, 0)])
    # one by one they work: a drop-in Evaluate reads its own reading submap's layout
    n = cfs[0].num_residuals()
    r = np.zeros(n)
    assert cfs[0].Evaluate([np.zeros(4), np.array([0.1, 0, 0, 0.02])], r, None) and np.abs(r).sum() > 0
    with pytest.raises(capi.VgxError):
        ctx.set_brick_layout(7)
    for o in cfs + [g0, g1]:
        o.destroy()
    ctx.close()


def test_a_sampling_batch_falls_back_to_apron_bricks_when_the_quad_copy_does_not_fit():
    """quad bricks on demand are the default for an all-sampling batch and cost 4.25 x the apron bricks per
    reading submap.  When that allocation fails the batch must still be created -- on the apron bricks, with the same
    results (the layout never shows in them) -- and the copies made for it so far must be given back.  The failure is
    simulated (VGX_TEST_QUAD_ALLOC_FAILS_AFTER=1: the second quad allocation of the process fails), in a child process
    because the switch is read once."""
    import os
    import subprocess
    import sys
    code = r"""
import numpy as np
from oracle import synth
from tests import helpers as H
from voxgraph_amd import capi
def world(sampling_bricks=None):
    ctx = capi.Context(0)
    if sampling_bricks is not None:
        ctx.set_sampling_bricks(sampling_bricks)
    ref, read = synth.config1_pair(asymmetric=True)
    subs = [H.gpu_submap(capi, ctx, sm, k) for k, sm in enumerate((ref, read))]
    for g in subs:
        g.extract_voxel_points(1.0, 0.3, True)
    return ctx, subs
poses = np.array([[0.02, -0.01, 0.03, 0.01], [0.31, -0.2, 0.08, 0.12]])
def run(ctx, subs):
    cfg = capi.default_config(registration_point_type=capi.POINTS_VOXELS, sampling_ratio=0.3, sampler_seed=7)
    cfs = [capi.RegistrationCostFunction(ctx, subs[a], subs[b], cfg) for a, b in ((0, 1), (1, 0))]
    batch = capi.RegistrationBatch(ctx, cfs, [(0, 1), (1, 0)])      # two reading submaps: the second quad copy "fails"
    layout = batch.brick_layout()
    status, normal = batch.evaluate_normal(poses)
    return layout, normal
ctx, subs = world()
layout, normal = run(ctx, subs)
assert layout == capi.BRICKS_APRON, layout
ctx2, subs2 = world(capi.SAMPLING_BRICKS_SAME)
layout2, normal2 = run(ctx2, subs2)
assert layout2 == capi.BRICKS_APRON and np.array_equal(normal, normal2) and np.abs(normal).max() > 0
print("fallback ok")
"""
    env = dict(os.environ, VGX_TEST_QUAD_ALLOC_FAILS_AFTER="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fallback ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    assert "reads the apron bricks" in r.stderr
