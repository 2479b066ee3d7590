"""The map-evaluation restatement (tests/map_eval_ref.py) on hand-built cases whose answer is known by construction:
evaluateLayersRmse's block and voxel classes in every mode, the fixed f64 association, the min_error quirk, and
transformLayer on an exact whole-block shift (voxel size 0.25: every coordinate dyadic)."""
import numpy as np
import pytest

from oracle.synth import SubmapData
from tests import map_eval_ref as R
from tests import projected_map_ref as P

F = np.float32


def _layer(blocks, vps, d, obs):
    n = len(blocks)
    return R.esdf_layer(np.array(blocks, np.int64).reshape(n, 3), np.broadcast_to(np.asarray(d, F), (n, vps ** 3)).copy(),
                        np.broadcast_to(np.asarray(obs, bool), (n, vps ** 3)).copy())


@pytest.mark.parametrize("vps", [8, 16])
def test_blocks_only_on_one_side_are_non_overlapping(vps):
    nv = vps ** 3
    gt = _layer([(0, 0, 0), (1, 0, 0)], vps, 0.5, True)
    test = _layer([(0, 0, 0), (0, 2, 0), (5, 5, 5)], vps, 0.75, True)
    det, (bi, e, st) = R.evaluate_layers_rmse(gt, test, R.ALL_VOXELS, vps)
    assert det["num_non_overlapping_voxels"] == 3 * nv      # gt (1,0,0); test (0,2,0) and (5,5,5)
    assert det["num_evaluated_voxels"] == nv and det["num_overlapping_voxels"] == nv
    assert det["total_squared_error"] == nv * 0.0625 and det["rmse"] == 0.25
    assert bi.tolist() == [[0, 0, 0]] and (e == F(0.25)).all() and (st == 1).all()


def test_unobserved_voxels_on_either_side_do_not_overlap():
    vps, nv = 8, 512
    og = np.ones(nv, bool)
    ot = np.ones(nv, bool)
    og[:10] = False
    ot[5:30] = False                                     # 30 voxels unobserved on one side or both
    gt = R.esdf_layer([[0, 0, 0]], np.full((1, nv), 1.0, F), og[None])
    test = R.esdf_layer([[0, 0, 0]], np.full((1, nv), 1.5, F), ot[None])
    det, (_, e, st) = R.evaluate_layers_rmse(gt, test, R.ALL_VOXELS, vps)
    assert det["num_non_overlapping_voxels"] == 30 and det["num_evaluated_voxels"] == nv - 30
    assert (st[0, :30] == 0).all() and (e[0, :30] == 0).all() and (st[0, 30:] == 1).all()
    # a TSDF layer counts a voxel as observed when its weight exceeds 1e-6
    w = np.full((1, nv), 2e-6, F)
    w[0, :7] = F(1e-6)
    t = R.tsdf_layer([[0, 0, 0]], np.zeros((1, nv), F), w)
    det, _ = R.evaluate_layers_rmse(t, t, R.ALL_VOXELS, vps)
    assert det["num_non_overlapping_voxels"] == 7 and det["num_evaluated_voxels"] == nv - 7 and det["rmse"] == 0.0


@pytest.mark.parametrize("mode,ignored", [(R.ALL_VOXELS, 0), (R.IGNORE_BEHIND_TEST, 2), (R.IGNORE_BEHIND_GT, 2),
                                          (R.IGNORE_BEHIND_ALL, 3)])
def test_negative_distances_in_each_mode(mode, ignored):
    vps, nv = 8, 512
    dg = np.full(nv, 1.0, F)
    dt = np.full(nv, 1.0, F)
    dt[0], dg[1] = -0.5, -0.5                 # behind the test surface; behind the gt surface
    dt[2], dg[2] = -0.25, -0.75               # behind both
    gt = R.esdf_layer([[0, 0, 0]], dg[None], np.ones((1, nv), bool))
    test = R.esdf_layer([[0, 0, 0]], dt[None], np.ones((1, nv), bool))
    det, (_, e, st) = R.evaluate_layers_rmse(gt, test, mode, vps)
    behind = {R.ALL_VOXELS: [], R.IGNORE_BEHIND_TEST: [0, 2], R.IGNORE_BEHIND_GT: [1, 2], R.IGNORE_BEHIND_ALL: [0, 1, 2]}[mode]
    assert det["num_ignored_voxels"] == ignored == len(behind)
    assert det["num_evaluated_voxels"] == nv - ignored and det["num_overlapping_voxels"] == nv
    errs = {0: 1.5, 1: 1.5, 2: 0.5}
    want = sum(errs[i] ** 2 for i in errs if i not in behind)
    assert det["total_squared_error"] == want
    assert det["max_error"] == (1.5 if want > 0.5 else (0.5 if want else 0.0))
    for i in range(3):
        assert st[0, i] == (i not in behind) and e[0, i] == (0 if i in behind else dt[i] - dg[i])


def test_nothing_evaluated_gives_rmse_zero():
    vps, nv = 8, 512
    gt = _layer([(0, 0, 0)], vps, 1.0, False)
    test = _layer([(0, 0, 0)], vps, 1.0, True)
    det, (bi, e, st) = R.evaluate_layers_rmse(gt, test, R.ALL_VOXELS, vps)
    assert det["num_evaluated_voxels"] == 0 and det["rmse"] == 0.0 and det["total_squared_error"] == 0.0
    assert det["min_abs_error"] == 0.0 and det["max_error"] == 0.0 and det["num_non_overlapping_voxels"] == nv
    assert len(bi) == 1 and not st.any()         # the error block exists (the test block has a gt counterpart)
    det, (bi, _, _) = R.evaluate_layers_rmse(_layer([], vps, 0, True), _layer([], vps, 0, True), R.ALL_VOXELS, vps)
    assert det["rmse"] == 0.0 and det["num_non_overlapping_voxels"] == 0 and len(bi) == 0


def test_min_error_quirk_reports_zero_and_the_true_minimum_separately():
    vps, nv = 8, 512
    gt = _layer([(0, 0, 0)], vps, 1.0, True)
    dt = np.full(nv, 1.5, F)
    dt[77] = 1.125
    test = R.esdf_layer([[0, 0, 0]], dt[None], np.ones((1, nv), bool))
    det, _ = R.evaluate_layers_rmse(gt, test, R.ALL_VOXELS, vps)
    assert det["min_error"] == 0.0 and det["min_abs_error"] == 0.125 and det["max_error"] == 0.5


def test_sum_association_is_the_stated_one():
    """The restated sum is the tree the header describes, not numpy's pairwise sum: on values spanning many binades the
    two orders differ, and the stated one is reproduced by a plain transcription of the loop."""
    rng = np.random.default_rng(3)
    vps, nv = 16, 4096
    sq = (rng.random((3, nv)) * 10.0 ** rng.integers(-8, 4, (3, nv)))
    got = R.block_sums(sq, vps)
    for b in range(3):
        per_thread = [0.0] * 256
        for k in range(4):
            for t in range(256):
                for j in range(4):
                    per_thread[t] += sq[b, 4 * (t + 256 * k) + j]
        waves = []
        for w in range(4):
            lanes = per_thread[64 * w:64 * w + 64]
            o = 32
            while o:
                lanes = [lanes[i] + lanes[i + o] if i < o else lanes[i] for i in range(64)]
                o //= 2
            waves.append(lanes[0])
        acc = waves[0]
        for v in waves[1:]:
            acc += v
        assert got[b] == acc
    p = rng.random(3000) * 10.0 ** rng.integers(-8, 4, 3000)
    th = [0.0] * 1024
    for i, v in enumerate(p):
        th[i % 1024] += v
    waves = []
    for w in range(16):
        lanes = th[64 * w:64 * w + 64]
        o = 32
        while o:
            lanes = [lanes[i] + lanes[i + o] if i < o else lanes[i] for i in range(64)]
            o //= 2
        waves.append(lanes[0])
    acc = waves[0]
    for v in waves[1:]:
        acc += v
    assert R.fold_sums(p) == acc


def _grid_submap(vps, vs, seed):
    rng = np.random.default_rng(seed)
    bi = np.array([(x, y, z) for x in range(3) for y in range(3) for z in range(3)], np.int32)
    d = rng.uniform(-0.5, 0.5, (len(bi), vps ** 3)).astype(F)
    w = rng.uniform(0.5, 20.0, (len(bi), vps ** 3)).astype(F)
    return SubmapData(vs, vps, bi, d, w, np.zeros_like(d), np.zeros(d.shape, np.uint8), np.zeros(4))


def test_transform_exact_whole_block_shift():
    vps, vs = 8, 0.25
    sm = _grid_submap(vps, vs, 5)
    shift = np.array([1, -2, 3])
    T = np.array([1, 0, 0, 0, *(shift * vps * vs)], F)
    out = R.transform_layer(sm, T)
    assert set(out) == {tuple(int(c) for c in b + shift) for b in sm.block_index}
    i = np.arange(vps ** 3)
    vx, vy, vz = i % vps, (i // vps) % vps, i // (vps * vps)
    for b, d, w in zip(sm.block_index, sm.tsdf_distance, sm.tsdf_weight):
        od, ow = out[tuple(int(c) for c in b + shift)]
        # a voxel interpolates iff its +1 neighbours exist: all but the max faces of the 3 x 3 x 3 block region
        edge = ((b[0] == 2) & (vx == vps - 1)) | ((b[1] == 2) & (vy == vps - 1)) | ((b[2] == 2) & (vz == vps - 1))
        assert np.array_equal(od[~edge].view(np.uint32), d[~edge].view(np.uint32))
        assert np.array_equal(ow[~edge].view(np.uint32), w[~edge].view(np.uint32))
        assert not od[edge].any() and not ow[edge].any()


def test_transform_copies_where_a_merge_into_an_empty_layer_would_round():
    vps, vs = 8, 0.25
    sm = _grid_submap(vps, vs, 6)
    T = np.array([np.cos(0.15), 0, 0, np.sin(0.15), 0.3, -0.2, 0.1], F)
    copied = R.transform_layer(sm, T)
    merged = P.merge_one({}, sm, T)
    assert set(copied) == set(merged) and len(copied) > 20
    w_same = all(np.array_equal(copied[k][1], merged[k][1]) for k in copied)
    d_diff = sum(int((copied[k][0].view(np.uint32) != merged[k][0].view(np.uint32)).sum()) for k in copied)
    assert w_same and d_diff > 0
