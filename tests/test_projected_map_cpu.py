"""The projected map's CPU restatement (tests/projected_map_ref.py) pinned to the existing C oracle: the inverse and the
transform to orc_transform_point, the interpolation to orc_get_voxels_and_q on a distance and a weight layer combined
in iso_oracle.c's association -- exactly, at thousands of positions.  Plus properties of the merge.  No GPU."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import projected_map_ref as pm

F = np.float32

# iso_oracle.c: interpolation coefficients of the 8 neighbours
B = np.array([[1, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 1, 0, 0, 0], [-1, 0, 1, 0, 0, 0, 0, 0],
              [-1, 1, 0, 0, 0, 0, 0, 0], [1, 0, -1, 0, -1, 0, 1, 0], [1, -1, -1, 1, 0, 0, 0, 0],
              [1, -1, 0, 0, -1, 1, 0, 0], [-1, 1, 1, -1, 1, -1, -1, 1]], F)


def _unit_quat(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(F)


def _poses(rng):
    yaw = 0.7
    out = [np.array([1, 0, 0, 0, 0, 0, 0], F),
           np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), 1.3, -2.1, 0.4], F)]
    for _ in range(4):
        out.append(np.concatenate([_unit_quat(rng), rng.uniform(-20, 20, 3)]).astype(F))
    return out


def test_inverse_and_transform_match_the_oracle():
    rng = np.random.default_rng(1)
    pts = rng.uniform(-50, 50, (2000, 3)).astype(F)
    for T in _poses(rng):
        qi, ti = pm.inverse(T)
        # the oracle's form of inverse(): conjugate, then -(q^-1 t) through orc_transform_point with t = 0
        q_conj = np.array([T[0], -T[1], -T[2], -T[3]], F)
        t_ref = -orc.transform_point(q_conj, np.zeros(3, F), T[4:7])
        assert np.array_equal(qi, q_conj) and np.array_equal(ti, t_ref)
        got = pm.transform(qi, ti, pts)
        want = np.stack([orc.transform_point(qi, ti, p) for p in pts])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _random_raw_layer(rng, vps, voxel_size, n_blocks=14):
    # a compact random block set around the origin (negative coordinates included), holes between blocks
    cand = np.array([(x, y, z) for x in range(-2, 2) for y in range(-2, 1) for z in range(-1, 2)], np.int32)
    bi = cand[rng.choice(len(cand), n_blocks, replace=False)]
    nv = vps ** 3
    d = rng.uniform(-0.5, 0.5, (n_blocks, nv)).astype(F)
    w = rng.uniform(0.1, 20, (n_blocks, nv)).astype(F)
    w[rng.random(w.shape) < 0.03] = 0                  # invalid neighbours
    return type("Sm", (), dict(voxel_size=float(F(voxel_size)), vps=vps, block_index=bi, tsdf_distance=d,
                               tsdf_weight=w))


def _oracle_interp(Ld, Lw, p):
    okd, d8, q = Ld.voxels_and_q(p)
    okw, w8, _ = Lw.voxels_and_q(p)
    if not (okd and okw):
        return False, F(0), F(0)
    di, wi = F(0), F(0)
    for r in range(8):
        cd, cw = F(0), F(0)
        for k in range(8):
            cd = F(cd + F(B[r, k] * d8[k]))
            cw = F(cw + F(B[r, k] * w8[k]))
        di = F(di + F(q[r] * cd))
        wi = F(wi + F(q[r] * cw))
    return True, di, wi


@pytest.mark.parametrize("vps,voxel_size", [(16, 0.1), (8, 0.2)])
def test_interpolation_matches_the_oracle(vps, voxel_size):
    rng = np.random.default_rng(vps)
    sm = _random_raw_layer(rng, vps, voxel_size)
    raw = pm.RawLayer(sm)
    valid = sm.tsdf_weight > 0
    Ld = orc.Layer(sm.voxel_size, vps, sm.block_index, sm.tsdf_distance, valid)
    Lw = orc.Layer(sm.voxel_size, vps, sm.block_index, sm.tsdf_weight, valid)
    bs = F(vps) * F(voxel_size)
    lo = sm.block_index.min(0).astype(F) * bs
    hi = (sm.block_index.max(0) + 1).astype(F) * bs
    p_free = rng.uniform(lo - bs / 4, hi + bs / 4, (2500, 3)).astype(F)
    # block faces and voxel centres exactly, and points a hair off them
    faces = rng.uniform(lo, hi, (600, 3)).astype(F)
    axis = rng.integers(0, 3, 600)
    faces[np.arange(600), axis] = (np.round(faces[np.arange(600), axis] / bs) * bs).astype(F)
    centres = pm.block_centres(sm.block_index[:3], vps, voxel_size).reshape(-1, 3)[::7][:400]
    nudged = np.nextafter(centres, F(np.inf)).astype(F)
    pts = np.concatenate([p_free, faces, centres, nudged]).astype(F)
    ok, d, w = raw.interp(pts)
    n_ok = 0
    for i, p in enumerate(pts):
        ok0, d0, w0 = _oracle_interp(Ld, Lw, p)
        assert ok[i] == ok0, (i, p)
        if ok0:
            n_ok += 1
            assert d[i] == d0 and w[i] == w0, (i, p, d[i], d0, w[i], w0)
    assert n_ok > 500 and (~ok).sum() > 300


def test_merge_rule():
    rng = np.random.default_rng(3)
    db = rng.uniform(-1, 1, 1000).astype(F)
    wb = rng.uniform(0, 5, 1000).astype(F)
    wb[:100] = 0
    # merging the default voxel (0, 0): weight unchanged; distance (0 * 0 + d w) / w, which need not be d
    d1, w1 = pm.merge_voxels(np.zeros_like(db), np.zeros_like(wb), db, wb)
    assert np.array_equal(w1, wb)
    assert np.array_equal(d1[:100], db[:100])                      # w' = 0: unchanged
    assert np.array_equal(d1[100:], ((db * wb) / wb)[100:].astype(F))
    # weights add, distance is the weighted mean in f32
    da = rng.uniform(-1, 1, 1000).astype(F)
    wa = rng.uniform(0.5, 5, 1000).astype(F)
    d2, w2 = pm.merge_voxels(da, wa, db, wb)
    assert np.array_equal(w2, (wa + wb).astype(F))
    assert np.array_equal(d2, (((da * wa) + (db * wb)) / (wa + wb)).astype(F))
    assert np.all(np.minimum(da, np.where(wb > 0, db, da)) - 1e-6 <= d2)
    assert np.all(d2 <= np.maximum(da, np.where(wb > 0, db, da)) + 1e-6)
    # order matters in the last bits (merge is not associative in f32), not in the weights
    dc, wc = rng.uniform(-1, 1, 1000).astype(F), rng.uniform(0.5, 5, 1000).astype(F)
    x = pm.merge_voxels(dc, wc, *pm.merge_voxels(da, wa, db, wb))
    y = pm.merge_voxels(da, wa, *pm.merge_voxels(dc, wc, db, wb))
    assert np.allclose(x[0], y[0], atol=1e-6) and np.allclose(x[1], y[1], rtol=1e-6)


def test_identity_projection_of_one_submap_into_an_empty_layer():
    """T = identity: every layer voxel centre IS a source voxel centre; a voxel interpolates iff its +x/+y/+z
    neighbourhood is valid, and then it merges to exactly (d w) / w of the source voxel."""
    rng = np.random.default_rng(5)
    sm = _random_raw_layer(rng, 8, 0.2)
    layer = pm.merge_submaps({}, [sm], np.array([[1, 0, 0, 0, 0, 0, 0]], F))
    raw = pm.RawLayer(sm)
    for key, (d, w) in layer.items():
        c = pm.block_centres(np.array([key]), 8, sm.voxel_size)[0]
        ok, di, wi = raw.interp(c)
        assert ok.any()
        s = raw.slot(np.array(key))
        if s >= 0:
            assert np.array_equal(di[ok], sm.tsdf_distance[s][ok]) and np.array_equal(wi[ok], sm.tsdf_weight[s][ok])
        assert np.array_equal(w, np.where(ok, wi, F(0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(d[ok], ((di * wi) / wi)[ok].astype(F))
