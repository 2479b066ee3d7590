"""Scan undistortion without a GPU: the numpy restatement (tests/scan_undistort_ref.py) that the GPU tests compare the
kernel with, against answers known another way -- the plain decode under an identity knot, a per-stamp rigid transform
when every stamp is a knot, np.searchsorted for the segment, the f64 closed form of a moving sensor's sweep -- and every
refusal of the host-only vgx_scan_undistort_check."""
import numpy as np
import pytest

from tests import scan_msg_ref as R
from tests import scan_undistort_ref as U
from tests import scan_undistort_scenes as Z

F = np.float32
IDENTITY = np.array([[1, 0, 0, 0, 0, 0, 0]], F)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from voxgraph_amd import capi as m
    m.load()
    return m


@pytest.mark.parametrize("name", list(Z.LAYOUTS))
def test_an_identity_knot_is_the_plain_decode(name):
    """one knot (1,0,0,0, 0,0,0): every finite-time point comes back with its own value.  As VALUES: a -0.0 coordinate
    went through x + 1 * 0 + 0 + 0 and returns as +0.0, so the comparison is == on floats, not on bits."""
    m, f, xyz = Z.message(name, 211, 3, seed=1, row_pad=5)
    pts, rgba, kept = R.decode(m)
    got = U.decode(m, f, [0.05], IDENTITY)
    t = U.times(m, m.base()[kept], f)
    good = np.isfinite(t)
    assert got[3] == {"not_finite": m.n - len(kept), "bad_time": int((~good).sum()), "overflowed": 0,
                      "clamped": int((t[good] != 0.05).sum())}
    assert (got[3]["bad_time"] > 0) == (f.kind != U.TIME_UINT32) and got[3]["not_finite"] > 10
    assert np.array_equal(got[2], kept[good]) and np.array_equal(got[1], rgba[good])
    assert np.array_equal(got[0], pts[good]) and (np.signbit(pts[good]) & (pts[good] == 0)).any()
    assert not (np.signbit(got[0]) & (got[0] == 0)).any()


def test_a_knot_at_every_stamp_is_one_rigid_transform_per_stamp():
    m, f, _ = Z.message("driver48", 64, 40, seed=2)
    stamps = np.arange(64) * 1.5e-3 + 2e-3
    Z.put_time(m, f, Z.raw_times(f, np.tile(stamps, 40)))
    kt = np.unique(U.times(m, m.base(), f))
    assert len(kt) == 64
    kT = Z.knots(m, f, 64, seed=2)[1]
    pts, rgba, kept = R.decode(m)
    got = U.decode(m, f, kt, kT)
    want = U.transform_point(kT[kept % 64], pts)
    assert got[3] == {"not_finite": m.n - len(kept), "bad_time": 0, "overflowed": 0, "clamped": 0}
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[2], kept)
    assert np.abs(want - pts).max() > 0.05


def test_transform_point_by_hand():
    """a quarter turn about z and a translation: (1, 2, 3) -> (-2, 1, 3) + (10, 20, 30), to f32 rounding of sqrt(1/2)"""
    s = np.sqrt(0.5)
    g = U.transform_point(np.array([s, 0, 0, s, 10, 20, 30], F), np.array([[1, 2, 3]], F))
    assert np.abs(g - [[8, 21, 33]]).max() < 4e-6
    assert np.array_equal(U.transform_point(IDENTITY, np.array([[1.5, -2.25, 0.0]], F)), [[1.5, -2.25, 0.0]])


def test_segment_rule_matches_searchsorted_at_and_around_the_knots():
    kt = np.array([0.01, 0.02, 0.02 + 1e-12, 0.05, 0.09])
    below, above = np.nextafter(kt, -np.inf), np.nextafter(kt, np.inf)
    t = np.concatenate([kt, below, above, [-1.0, 0.0, 0.0999, 1e9, 0.03]])
    k, a, clamped = U.segment(t, kt)
    cnt = np.searchsorted(kt, t, side="right")
    assert np.array_equal(k, np.maximum(cnt - 1, 0))
    assert k[:5].tolist() == [0, 1, 2, 3, 4] and not clamped[:5].any() and (a[:5] == 0).all()       # at a knot: a = 0
    assert k[5:10].tolist() == [0, 0, 1, 2, 3] and clamped[5:10].tolist() == [True, False, False, False, False]
    assert a[5] == 0 and (a[6:10] > 0.99).all() and (a[6:10] <= 1).all()                             # just below a knot
    assert k[10:15].tolist() == [0, 1, 2, 3, 4] and clamped[10:15].tolist() == [False] * 4 + [True]
    assert (a[10:14] > 0).all() and (a[10:14] < 1e-3).all() and a[14] == 0                           # just above a knot
    assert k[15:].tolist() == [0, 0, 4, 4, 2] and clamped[15:].tolist() == [True, True, True, True, False]
    assert a[-1] == F((0.03 - kt[2]) / (0.05 - kt[2])) and (a[15:19] == 0).all()
    # one knot: everything but the knot's own time is clamped
    k, a, clamped = U.segment(np.array([0.0, 0.5, 1.0]), [0.5])
    assert k.tolist() == [0, 0, 0] and (a == 0).all() and clamped.tolist() == [True, False, True]


def test_blend_by_hand():
    """two knots that differ by a translation: a point a quarter of the way gets a quarter of it; at a == 0 the second
    knot is not evaluated (it would overflow)"""
    kT = np.array([[1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 4, -8, 16]], F)
    p = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1]], F)
    out, clamped = U.undistort_points(p, np.array([0.25, 0.0, 1.0]), [0.0, 1.0], kT)
    assert out.tolist() == [[2, -1, 5], [1, 1, 1], [5, -7, 17]] and not clamped.any()
    s = np.sqrt(0.5)
    kT = np.array([[1, 0, 0, 0, 0, 0, 0], [s, 0, 0, s, 0, 0, 0]], F)
    big = np.array([[3e38, 3e38, 0]] * 3, F)
    out, clamped = U.undistort_points(big, np.array([-1.0, 0.0, 0.5]), [0.0, 1.0], kT)
    assert np.isfinite(out[:2]).all() and not np.isfinite(out[2]).all() and clamped.tolist() == [True, False, False]


def test_overflow_scene_counts():
    m, f, kt, kT = Z.overflow_scene()
    pts, rgba, kept, stats = U.decode(m, f, kt, kT)
    big = np.arange(10, 300, 7)
    survive = big[big % 2 == 0]                                          # before the track: the identity knot alone
    assert stats == {"not_finite": 0, "bad_time": 0, "overflowed": len(big) - len(survive), "clamped": 150 + 75 - int((big % 4 == 1).sum())}
    assert stats["overflowed"] > 10 and np.isin(survive, kept).all() and not np.isin(np.setdiff1d(big, survive), kept).any()
    assert np.isfinite(pts).all() and (np.abs(pts) > 1e38).any()


def test_every_refusal_of_undistort_check(capi):
    m, f, _ = Z.message("step36_f64_at20", 10, 2)
    lay, need = m.layout(capi), len(m.data)
    kt, kT = np.array([0.0, 0.5, 1.0]), np.array([[1, 0, 0, 0, 0, 0, 0]] * 3, F)
    ok, inv, uns = capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED

    def check(layout=lay, n_bytes=need, kt=kt, kT=kT, **tf):
        d = dict(kind=f.kind, offset=f.offset, scale=f.scale, offset_s=f.offset_s)
        d.update(tf)
        return capi.scan_undistort_check(layout, capi.scan_time_field(**d), kt, kT, n_bytes)

    assert check() == ok
    assert capi.scan_undistort_check(None, f.capi(capi), kt, kT, need) == inv
    assert capi.scan_undistort_check(lay, None, kt, kT, need) == inv
    assert capi.scan_undistort_check(lay, f.capi(capi), None, None, need) == inv
    view = capi.ScanTrackView(3, None, None)
    assert capi.load().vgx_scan_undistort_check(lay, f.capi(capi), view, need) == inv      # NULL knot arrays
    assert check(kind=3) == inv and check(kind=-1) == inv
    # the time field must fit: 8 bytes at 28 fit in 36, at 29 they do not; 4 bytes fit at 32, not at 33
    assert check(offset=28) == ok and check(offset=29) == inv and check(offset=0xfffffffc) == inv
    assert check(kind=U.TIME_FLOAT32, offset=32) == ok and check(kind=U.TIME_UINT32, offset=33) == inv
    for bad in (np.nan, np.inf, -np.inf):
        assert check(scale=bad) == inv and check(offset_s=bad) == inv
    assert check(kt=[], kT=np.zeros((0, 7))) == inv                                        # n_knots 0
    view, keep = capi.scan_track_view(kt, kT)
    view.n_knots = -1
    assert capi.load().vgx_scan_undistort_check(lay, f.capi(capi), view, need) == inv
    big = 65537
    assert check(kt=np.arange(big, dtype=np.float64), kT=np.tile(kT[:1], (big, 1))) == inv
    assert check(kt=np.arange(big - 1, dtype=np.float64), kT=np.tile(kT[:1], (big - 1, 1))) == ok
    assert check(kt=[0.5], kT=kT[:1]) == ok
    for bad_kt in ([0.0, 0.5, 0.5], [0.0, 1.0, 0.5], [0.0, np.nan, 1.0], [-np.inf, 0.5, 1.0], [0.0, 0.5, np.inf]):
        assert check(kt=bad_kt) == inv, bad_kt
    for j in range(7):
        for bad in (np.nan, np.inf):
            bad_T = kT.copy()
            bad_T[2, j] = bad
            assert check(kT=bad_T) == inv
    # everything the plain decode refuses
    assert check(n_bytes=need - 1) == inv and check(n_bytes=-1) == inv

    def layout(**kw):
        l2 = m.layout(capi)
        for k, v in kw.items():
            setattr(l2, k, v)
        return l2

    assert check(layout=layout(point_step=0)) == inv and check(layout=layout(offset_z=33)) == inv
    assert check(layout=layout(row_step=359)) == inv and check(layout=layout(color_kind=5)) == inv
    assert check(layout=layout(is_bigendian=1)) == uns


def test_track_helper_by_hand(capi):
    """relative_to: the reference itself gives the identity; a sensor one metre ahead of a reference that is turned a
    quarter turn about z lies at (0, -1, 0) ... in the reference's frame, turned back by the quarter turn"""
    s = np.sqrt(0.5)
    tr = capi.ScanTrack()
    ref = [s, 0, 0, s, 1.0, 2.0, 3.0]
    tr.add(10.0, ref)
    tr.add(10.5, [1, 0, 0, 0, 2.0, 2.0, 3.0])
    tr.add(11.0, [2 * s, 0, 0, 2 * s, 1.0, 2.0, 4.0])                   # (not normalised: the helper normalises)
    kt, kT = tr.relative_to(ref, stamp=10.0)
    assert kt.tolist() == [0.0, 0.5, 1.0] and kT.dtype == F and kT.shape == (3, 7)
    want = np.array([[1, 0, 0, 0, 0, 0, 0], [s, 0, 0, -s, 0, -1, 0], [1, 0, 0, 0, 0, 0, 1]])
    assert np.abs(kT - want).max() < 1e-7


BOX_LO, BOX_HI = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])     # the room of scan_msg_scenes._room_hits
SWEEP_S, ROWS, COLS = 0.1, 64, 1024


def moving_sweep(capi, seed):
    """A 64 x 1024 sweep of the box room by a sensor at constant 2 m/s and 1 rad/s (about z), no noise: column c fires
    at t_c = 0.1 s * c / 1024, its points are expressed in the sensor frame at t_c (f32), the reference time is the
    sweep's end.  Everything else in f64.  -> (points, t per point, truth = T_ref^-1 * hit, a track builder)"""
    heading = 0.7 * seed
    vel = 2.0 * np.array([np.cos(heading), np.sin(heading), 0.0])

    def pose(t):
        t = np.asarray(t, np.float64)
        z = np.zeros_like(t)
        return np.stack([np.cos(0.5 * t), z, z, np.sin(0.5 * t), vel[0] * t, vel[1] * t, vel[2] * t + z], -1)

    def rot(t):
        c, s, z, o = np.cos(t), np.sin(t), np.zeros_like(t), np.ones_like(t)
        return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)

    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, COLS, endpoint=False) + (2 * np.pi / COLS) / 3.0 + 0.01 * seed,
                         np.linspace(-0.3, 0.3, ROWS) + 0.004)
    t = np.tile(SWEEP_S * np.arange(COLS) / COLS, ROWS)
    d_s = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    Rt = rot(1.0 * t)
    d_w = np.einsum("nij,nj->ni", Rt, d_s)
    pos = vel[None, :] * t[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        reach = np.where(d_w > 0, (BOX_HI - pos) / d_w, np.where(d_w < 0, (BOX_LO - pos) / d_w, np.inf)).min(1)
    hit = pos + d_w * reach[:, None]
    p_s = np.einsum("nji,nj->ni", Rt, hit - pos).astype(F)
    truth = (hit - vel * SWEEP_S) @ rot(np.float64(SWEEP_S))             # R_ref^T (hit - pos_ref), as a row vector product

    def track(every):
        cols = np.arange(0, COLS, every)
        kt = np.concatenate([SWEEP_S * cols / COLS, [SWEEP_S]]) if every > 1 else SWEEP_S * cols / COLS
        tr = capi.ScanTrack()
        for tk, Tk in zip(kt, pose(kt)):
            tr.add(tk, Tk)
        return tr.relative_to(pose(SWEEP_S))
    return p_s, t, truth, track


# The worst distance between the restatement's output and the f64 closed form over seeds 0 .. 5, measured (the
# restatement is deterministic: the factor 2 below is for seeds not tried):
#   a knot at every column     8.26e-07 m   (f32 rounding of points up to 8 m away and of the knots)
#   a knot every 16 columns    2.21e-06 m   (plus the chord's sag, r * dtheta^2 / 8 with dtheta = 1.56 mrad)
WORST_EVERY_COLUMN, WORST_EVERY_16 = 8.26e-07, 2.21e-06


@pytest.mark.parametrize("seed", range(6))
def test_a_moving_sensors_sweep_is_undistorted_to_the_closed_form(capi, seed):
    p, t, truth, track = moving_sweep(capi, seed)
    raw = np.linalg.norm(p.astype(np.float64) - truth, axis=1).max()
    for every, worst in ((1, WORST_EVERY_COLUMN), (16, WORST_EVERY_16)):
        kt, kT = track(every)
        assert len(kt) == (COLS if every == 1 else COLS // every + 1)
        out, clamped = U.undistort_points(p, t, kt, kT)
        err = np.linalg.norm(out.astype(np.float64) - truth, axis=1).max()
        print(f"seed {seed} knots every {every}: worst {err:.3e} m, raw cloud {raw:.3e} m")
        assert err <= 2 * worst and not clamped.any()
        assert raw >= 100 * err and raw > 0.1                            # (an identity would leave the raw cloud's error)
