"""The map-query restatement (tests/map_query_ref.py) on hand-built layers whose answer is known by construction: a
linear field (interpolation exact, the gradient its slope), one unobserved neighbour, block faces and negative
coordinates, the 1e-6 epsilon on voxel centres and block faces, and non-finite points."""
import numpy as np
import pytest

from oracle.synth import SubmapData
from tests import map_query_ref as R

F = np.float32
SLOPE = np.array([0.5, -0.25, 0.125], F)  # dyadic: every product below is exact in f32


def _layer(vps, blocks, voxel_size=0.25, field=None, observed=None):
    """a submap whose ESDF and TSDF both hold field(voxel centre), observed (weight 1) everywhere unless told otherwise"""
    bi = np.array(blocks, np.int32).reshape(-1, 3)
    i = np.arange(vps ** 3)
    idx = np.stack([i % vps, (i // vps) % vps, i // (vps * vps)], -1)
    c = ((bi[:, None, :] * vps + idx[None]).astype(np.float64) + 0.5) * voxel_size
    f = field if field is not None else (lambda p: p @ SLOPE.astype(np.float64) + 0.25)
    d = f(c).astype(F)
    obs = np.ones(d.shape, np.uint8) if observed is None else observed(c).astype(np.uint8)
    return SubmapData(voxel_size, vps, bi, d.copy(), obs.astype(F), d.copy(), obs, np.zeros(4))


def _cube(lo, hi):
    return [(x, y, z) for x in range(lo, hi) for y in range(lo, hi) for z in range(lo, hi)]


@pytest.mark.parametrize("vps", [8, 16])
@pytest.mark.parametrize("layer", ["esdf", "tsdf"])
def test_linear_field_is_interpolated_exactly_and_its_gradient_is_the_slope(vps, layer):
    sm = _layer(vps, _cube(-1, 1))
    rng = np.random.default_rng(1)
    ext = vps * 0.25
    p = rng.uniform(-ext + 0.6, ext - 0.6, (500, 3)).astype(F)  # every neighbour of every offset inside the 2x2x2 blocks
    d, g, w, ok = R.query(sm, p, layer, interpolate=True, gradient=True)
    assert ok.all()
    want = p.astype(np.float64) @ SLOPE.astype(np.float64) + 0.25
    np.testing.assert_allclose(d, want, atol=2e-6)
    np.testing.assert_allclose(g, np.broadcast_to(SLOPE, g.shape), atol=2e-5)
    if layer == "tsdf":
        np.testing.assert_allclose(w, 1.0, atol=1e-6)
    else:
        assert (w == 0).all()
    # nearest: the voxel's own value, and the gradient of a linear field sampled one voxel apart is the slope again
    d, g, _, ok = R.query(sm, p, layer, interpolate=False, gradient=True)
    assert ok.all()
    vc = (np.floor(p / F(0.25)) + 0.5) * 0.25
    np.testing.assert_allclose(d, vc @ SLOPE.astype(np.float64) + 0.25, atol=2e-6)
    np.testing.assert_allclose(g, np.broadcast_to(SLOPE, g.shape), atol=2e-5)


@pytest.mark.parametrize("layer", ["esdf", "tsdf"])
def test_one_unobserved_neighbour_fails_interpolation_but_not_the_nearest_voxel(layer):
    vps, vs = 8, 0.25
    hole = np.array([4, 4, 4])  # voxel (4,4,4) of block (0,0,0): centre (1.125)^3
    sm = _layer(vps, _cube(0, 1), vs, observed=lambda c: ~np.all(np.isclose(c, (hole + 0.5) * vs), -1))
    near_hole = np.array([[1.10, 1.10, 1.10]], F)  # a cube that has the hole as a corner; nearest voxel (4,4,4)
    next_to = np.array([[1.30, 1.20, 1.20]], F)    # nearest voxel (5,4,4): observed; interpolation reads the hole
    far = np.array([[0.4, 0.4, 0.4]], F)
    for p, interp_ok, nearest_ok in ((near_hole, False, False), (next_to, False, True), (far, True, True)):
        assert R.query(sm, p, layer, interpolate=True)[3][0] == interp_ok
        d, _, _, ok = R.query(sm, p, layer, interpolate=False)
        assert ok[0] == nearest_ok and (ok[0] or d[0] == 0)
    # a gradient fails when any of its six offsets does
    assert not R.query(sm, far + F(0.5), layer, interpolate=True, gradient=True)[3][0]


@pytest.mark.parametrize("vps", [8, 16])
def test_block_faces_and_negative_coordinates(vps):
    sm = _layer(vps, _cube(-2, 1))
    bs = vps * 0.25
    faces = np.array([[-bs, 0.1, -0.1], [-bs + 0.01, -bs - 0.01, 0.0], [0.0, 0.0, 0.0], [-0.125, -bs, -2 * bs + 0.45]], F)
    d, g, _, ok = R.query(sm, faces, "esdf", interpolate=True, gradient=True)
    assert ok.all()
    np.testing.assert_allclose(d, faces.astype(np.float64) @ SLOPE.astype(np.float64) + 0.25, atol=2e-6)
    np.testing.assert_allclose(g, np.broadcast_to(SLOPE, g.shape), atol=2e-5)
    # beyond the allocated blocks: invalid, zeros everywhere
    out = np.array([[bs + 0.2, 0, 0], [-2 * bs - 0.2, 0, 0], [0, 0, 50.0]], F)
    d, g, w, ok = R.query(sm, out, "tsdf", interpolate=True, gradient=True)
    assert not ok.any() and (d == 0).all() and (g == 0).all() and (w == 0).all()


def test_the_epsilon_decides_on_block_faces_and_voxel_centres():
    vps, vs = 8, 0.25
    sm = _layer(vps, [(0, 0, 0)], vs)  # block -1 absent
    # just below the face x = 0 the epsilon of floor(x / block_size + 1e-6) still says block 0
    p = np.array([[-1e-7, 0.5, 0.5], [-1e-3, 0.5, 0.5]], F)
    ok = R.query(sm, p, "esdf", interpolate=False)[3]
    assert ok.tolist() == [True, False]
    # a point on a voxel centre interpolates from that voxel upwards (p - centre < 0 is false): exactly its value
    c = np.array([[0.375, 0.625, 0.875]], F)
    d, _, _, ok = R.query(sm, c, "esdf", interpolate=True)
    assert ok[0] and d[0] == F(0.375 * 0.5 - 0.625 * 0.25 + 0.875 * 0.125 + 0.25)
    # on the face between two voxels: the nearest voxel is the upper one
    f = np.array([[0.5, 0.375, 0.375]], F)
    d = R.query(sm, f, "esdf", interpolate=False)[0]
    assert d[0] == F(0.625 * 0.5 - 0.375 * 0.25 + 0.375 * 0.125 + 0.25)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e30, -3e38])
def test_non_finite_and_huge_points_are_invalid(bad):
    sm = _layer(8, _cube(-1, 1))
    p = np.array([[0.1, 0.2, 0.3], [bad, 0.2, 0.3], [0.1, bad, 0.3], [0.1, 0.2, bad]], F)
    for interp in (False, True):
        d, g, w, ok = R.query(sm, p, "tsdf", interpolate=interp, gradient=True)
        assert ok.tolist() == [True, False, False, False]
        assert (d[1:] == 0).all() and (g[1:] == 0).all() and (w[1:] == 0).all()
        assert not np.signbit(d[1:]).any()


def test_a_pose_maps_points_into_the_submap_and_rotates_the_gradient_back():
    sm = _layer(8, _cube(-1, 1))
    yaw = np.pi / 2  # a quarter turn: the rotation is exact up to the quaternion's rounding
    T = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), 0.25, -0.5, 0.125], F)
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.8, 0.8, (200, 3)).astype(F)
    d, g, _, ok = R.query(sm, x, "esdf", interpolate=True, gradient=True, pose=T)
    # T_Q_S maps submap points s to x = R s + t: s = R^T (x - t), and the gradient in Q is R slope
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    s = (x.astype(np.float64) - T[4:].astype(np.float64)) @ Rz
    inside = (np.abs(s) < 2 - 0.6).all(1)
    assert ok[inside].all() and inside.sum() > 50
    np.testing.assert_allclose(d[inside], s[inside] @ SLOPE.astype(np.float64) + 0.25, atol=5e-6)
    np.testing.assert_allclose(g[inside], np.broadcast_to(Rz @ SLOPE.astype(np.float64), g[inside].shape), atol=5e-5)
