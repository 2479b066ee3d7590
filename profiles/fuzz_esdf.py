#!/usr/bin/env python3
"""Differential fuzzing of the device ESDF (vgx_submap_generate_esdf, voxgraph_submap.cpp:86): random small submaps, random
EsdfIntegrator settings (max / default / min distance), two scene families drawn by the seed:
  shell   oracle/synth.make_submap: spheres + ground observed within 2 * trunc of the surface only (8 / 16 voxels per side, blocks
          dropped at random, TSDF noise, unobserved holes) -- the front travels a few voxels at most, often not at all;
  carved  tests/esdf_scenes.carved_box: the same surfaces with the free space carved as an integrated layer has it (weight > 0,
          d = +-trunc everywhere, random holes, shuffled block rows) -- the front travels max_distance_m across several blocks.
Two comparisons per submap:
  1. tests/esdf_ref.py, the numpy restatement of the kernels (Jacobi sweeps in f32 to the fixed point): distance and observed
     layers equal BIT FOR BIT;
  2. oracle/esdf_oracle.c, the restated voxblox queue, which stops at improvements below min_diff_m = 1 mm where the device result
     is the EXACT fixed point: observed masks equal; fixed-band voxels the TSDF's values; the sign of every observed voxel the
     TSDF's; |gpu| <= |oracle| + 1e-6 and |gpu - oracle| < 4 mm (worst case reported: the queue's slack can add up, see BAR); the
     device layer satisfies the fixed-point equation to 1e-6 (tests/test_esdf_gpu.py's checker).  One stated exception: voxels on
     the max_distance_m frontier when default_distance_m lies beyond it (see below), counted.
draw() and queue_contract() need no device: tests/test_esdf_cpu.py holds the restatement to the queue over the same draws.
    SEEDS=200 python profiles/fuzz_esdf.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
# |device - queue| is NOT bounded by one min_diff_m: the queue's ignored improvements (< 1 mm each) can add up along a chain of
# voxels (seed 103822 of the first version of this fuzzer: 2.54 mm).  The fuzzer holds 4 mm and reports the worst case;
# tests/test_esdf_gpu.py's scenes stay below 2.5 mm.
BAR = 4e-3


def draw(seed):
    """-> (Scene or None when the draw holds no block, configuration keywords, description); no device needed"""
    from oracle import synth
    from tests import esdf_scenes as S
    rng = np.random.default_rng(seed)
    carved = bool(rng.integers(0, 2))
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.05, 0.1, 0.2]))
    dims = tuple(int(x) for x in rng.integers(1, 5 if vps == 8 or not carved else 4, 3))
    block_min = tuple(int(x) for x in rng.integers(-2, 2, 3))
    if carved:
        sc = S.carved_box(vps, vs, block_min, dims, int(rng.integers(0, 1 << 30)), holes=float(rng.choice([0.0, 0.05])))
        bi, td, tw = sc.bi, sc.td.copy(), sc.tw.copy()
    else:
        ext = np.array(dims) * vps * vs
        c = rng.uniform(0.2, 0.8, 3) * ext
        sdf = synth.sphere_ground_sdf(tuple(c), float(rng.uniform(0.2, 0.6) * ext.min()), float(rng.uniform(0.1, 0.4) * ext[2]))
        sm = synth.make_submap(sdf, vs, vps, block_min, dims, trunc=3 * vs, esdf_max=10 * vs, drop_empty_blocks=bool(rng.integers(0, 2)))
        bi, td, tw = sm.block_index, sm.tsdf_distance.copy(), sm.tsdf_weight.copy()
        if rng.integers(0, 2):
            tw = np.where(rng.uniform(size=tw.shape) < 0.03, 0, tw).astype(F)       # holes in the observed region
    if rng.integers(0, 2):
        td = np.clip(td + rng.normal(0, 0.02 * vs, td.shape).astype(F), -3 * vs, 3 * vs).astype(F)
    max_d = float(rng.choice([2.0, 6 * vs, 12 * vs]))
    kw = dict(max_distance_m=max_d, default_distance_m=float(rng.choice([max_d, 2.0])), min_distance_m=float(rng.choice([0.2, vs, 2 * vs])))
    what = dict(seed=seed, family="carved" if carved else "shell", vps=vps, vs=vs, dims=dims, blocks=len(bi), **kw)
    if len(bi) == 0:
        return None, kw, what
    return S.Scene(float(F(vs)), vps, np.ascontiguousarray(bi, np.int32), td, tw), kw, what


def queue_contract(sc, kw, ed, eo, od, oo):
    """(ed, eo): an exact fixed point (the device's layer or the restatement's); (od, oo): the queue's.  Asserts the contract of
    the module docstring; -> (worst |ed - od| off the frontier, frontier voxels that differ by more, fixed-point residual,
    observed voxels)"""
    from tests.test_esdf_gpu import _check_fixed_point
    td, tw = sc.td, sc.tw
    assert np.array_equal(eo, oo), "observed masks"
    obs = oo.astype(bool)
    fixed = (tw >= 1e-6) & (np.abs(td) < kw["min_distance_m"])
    assert np.array_equal(ed[fixed], td[fixed]), "fixed band"
    assert np.array_equal(np.sign(ed[obs]), np.sign(td[obs])), "signs"
    if not obs.any():
        return 0.0, 0, 0.0, 0
    # The frontier of max_distance_m when default_distance_m lies beyond it (not voxblox's defaults, 2 m / 2 m): a voxel is
    # reached only from a neighbour whose |distance| < max_distance_m, so where that neighbour sits within the queue's 1 mm
    # slack of the limit one side propagates (max + a step) and the other leaves the default -- a difference of
    # default - max, by construction of the two algorithms (seed 5840).  Counted, and required to be exactly that case.
    a_d, a_o = np.abs(ed), np.abs(od)
    lo = kw["max_distance_m"] - BAR
    # the shell beyond max_distance_m (it exists only when the default lies beyond the limit): a voxel there was reached from
    # a neighbour just below the limit; whether THAT neighbour is below it can differ by the queue's slack, and then the
    # voxel takes another neighbour's (longer) path or keeps the default (seeds 5840: default against 0.386 m; 111920: 7.4 mm)
    frontier_v = obs & (kw["default_distance_m"] > kw["max_distance_m"]) & ((a_d > lo) | (a_o > lo))
    assert np.all(np.minimum(a_d[frontier_v], a_o[frontier_v]) > lo - BAR), "a shell voxel on one side, an inner one on the other"
    frontier = int((frontier_v & (np.abs(ed - od) >= BAR)).sum())
    cmp_ = obs & ~frontier_v
    diff = np.abs(ed - od)[cmp_]
    assert diff.size == 0 or diff.max() < BAR, ("distance", float(diff.max()))
    assert np.all(np.abs(ed[cmp_]) <= np.abs(od[cmp_]) + 1e-6), "device above the queue's value"
    try:
        err, _ = _check_fixed_point(sc.bi, td, ed, eo, sc.vs, sc.vps, kw["min_distance_m"], kw["max_distance_m"], kw["default_distance_m"])
    except ValueError:          # (no observed voxel outside the fixed band: nothing propagates)
        err = 0.0
    assert err < 1e-6, ("fixed point", err)
    return (float(diff.max()) if diff.size else 0.0), frontier, err, int(obs.sum())


def main():
    from oracle import pyoracle as orc
    from tests import esdf_ref
    from voxgraph_amd import capi
    capi.load()
    ctx = capi.Context(0)
    n_seeds, first = int(os.environ.get("SEEDS", "100")), int(os.environ.get("FIRST", "0"))
    done, worst, worst_fp, voxels, frontier, propagating, moved = 0, 0.0, 0.0, 0, 0, 0, 0
    for seed in range(first, first + n_seeds):
        sc, kw, what = draw(seed)
        if sc is None:
            continue
        g = capi.Submap(ctx, 0, sc.vs, sc.vps, sc.bi, sc.td, sc.tw, None, None)
        try:
            g.generate_esdf(capi.esdf_config(**kw))
            _, _, ed, eo = g.download_layers(sc.vps)
            rd, ro = esdf_ref.esdf_from_tsdf(sc.vs, sc.vps, sc.bi, sc.td, sc.tw, kw["max_distance_m"], kw["min_distance_m"], kw["default_distance_m"])
            assert esdf_ref.same_bits(eo, ro), "observed layer against the restatement"
            assert esdf_ref.same_bits(ed, rd), ("distance layer against the restatement, voxels that differ", int((ed.view(np.uint32) != rd.view(np.uint32)).sum()))
            od, oo, _ = orc.esdf_from_tsdf(sc.vs, sc.vps, sc.bi, sc.td, sc.tw, orc.esdf_config(**kw))
            w, f, err, n_obs = queue_contract(sc, kw, ed, eo, od, oo)
            worst, worst_fp, frontier, voxels = max(worst, w), max(worst_fp, err), frontier + f, voxels + n_obs
            n_moved = int((eo.astype(bool) & ~(np.abs(sc.td) < kw["min_distance_m"]) & (np.abs(ed) < F(kw["default_distance_m"]))).sum())
            propagating, moved = propagating + (n_moved > 0), moved + n_moved
        except AssertionError as e:
            print("MISMATCH", what, str(e)[:300])
            return 1
        finally:
            g.destroy()
        done += 1
    print("no mismatch in %d submaps (%d observed voxels, every layer the restatement's bits; the front moved in %d submaps, %d voxels): "
          "worst |device - queue| %.2e m (bar %.1e), worst fixed-point residual %.1e; "
          "%d voxels of the shell beyond max_distance_m differ by more (default > max configurations only)" %
          (done, voxels, propagating, moved, worst, BAR, worst_fp, frontier))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
