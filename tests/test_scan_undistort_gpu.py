"""The undistorting scan decode (vgx_scan_decode_msg_undistorted, voxgraph_amd/csrc/vgx_scan.hip) against its numpy
restatement (tests/scan_undistort_ref.py), bit for bit: points as uint32, colours, order, the four counters; and what the
scan's consumers make of an undistorted scan against what they make of the restatement's arrays."""
import ctypes as C

import numpy as np
import pytest

from tests import scan_msg_ref as R
from tests import scan_msg_scenes as S
from tests import scan_undistort_ref as U
from tests import scan_undistort_scenes as Z

pytestmark = pytest.mark.gpu
F = np.float32


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


@pytest.fixture()
def scan(capi, ctx):
    s = capi.Scan(ctx)
    yield s
    s.destroy()


def _same(got, want):
    (gp, gc), (wp, wc) = got, want[:2]
    return (gp.shape == wp.shape and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)) and gc.shape == wc.shape
            and np.array_equal(gc, wc))


def _counters(m, want):
    st = want[3]
    return ((len(want[0]), st["not_finite"] + st["bad_time"] + st["overflowed"]), (st["bad_time"], st["overflowed"], st["clamped"]))


def _check(capi, scan, m, f, kt, kT, **cfg):
    want = U.decode(m, f, kt, kT, **cfg)
    got = scan.decode_undistorted(m.layout(capi), m.data, f.capi(capi), kt, kT, capi.scan_config(**cfg) if cfg else None)
    stats, ustats = _counters(m, want)
    assert got == stats and scan.stats() == stats and stats[0] + stats[1] == m.n
    assert scan.undistort_stats() == ustats
    assert _same(scan.download(), want)
    return want


def _check_plain(capi, scan, m):
    want = R.decode(m)
    assert scan.decode_msg(m.layout(capi), m.data) == (len(want[0]), m.n - len(want[0]))
    assert scan.undistort_stats() == (0, 0, 0) and _same(scan.download(), want)
    return want


CASES = [(name, 1031, 3, pad) for name in Z.LAYOUTS for pad in (0,)] + [("driver48", 50, 9, 24), ("step27_f32_at17", 50, 9, 5),
                                                                        ("step36_f64_at20", 77, 4, 4)]


@pytest.mark.parametrize("name,width,height,pad", CASES)
def test_layouts_equal_the_restatement(capi, scan, name, width, height, pad):
    m, f, _ = Z.message(name, width, height, seed=1, row_pad=pad)
    kt, kT = Z.knots(m, f, 64, seed=1)
    want = _check(capi, scan, m, f, kt, kT)
    st = want[3]
    assert st["not_finite"] >= 10 and st["clamped"] > 10 and (st["bad_time"] >= 3) == (f.kind != U.TIME_UINT32)
    # times met: at a knot (a == 0 inside the track), either side of one, before and after the track
    t = U.times(m, m.base()[want[2]], f)
    k, a, clamped = U.segment(t, kt)
    inside = ~clamped
    assert (a[inside] == 0).any() and (a[inside] > 0.9).any() and ((a[inside] > 0) & (a[inside] < 1e-6)).any()
    assert (t < kt[0]).any() and (t > kt[-1]).any()
    # another grey range and constant colour, on the same handle
    _check(capi, scan, m, f, kt, kT, intensity_min=-50.0, intensity_max=7000.0, constant_rgba=(1, 2, 3, 254))


@pytest.mark.parametrize("width,height", [(1, 1), (4, 1), (1023, 1), (1024, 1), (1025, 1), (4097, 1), (1031, 66)])
@pytest.mark.parametrize("name", ["driver48", "step27_f64_at19"])
def test_sizes(capi, scan, name, width, height):
    """one point, one thread's four, either side of a tile, several tiles, and 67 tiles: past the look-back's 64"""
    m, f, _ = Z.message(name, width, height, seed=2)
    kt, kT = Z.knots(m, f, 3, seed=2)
    _check(capi, scan, m, f, kt, kT)


@pytest.mark.parametrize("K", [1, 2, 3, 64, 1025, 65536])
def test_knot_counts(capi, scan, K):
    m, f, _ = Z.message("step36_f64_at20", 4097, 1, seed=3)
    kt, kT = Z.knots(m, f, K, seed=3)
    assert len(kt) == K
    want = _check(capi, scan, m, f, kt, kT)
    k = U.segment(U.times(m, m.base()[want[2]], f), kt)[0]
    assert k.min() == 0 and k.max() == K - 1 and len(np.unique(k)) >= min(K, 500)          # (many segments are met)


def test_points_that_overflow_under_a_quarter_turn(capi, scan):
    m, f, kt, kT = Z.overflow_scene()
    want = _check(capi, scan, m, f, kt, kT)
    assert want[3]["overflowed"] > 10 and (np.abs(want[0]) > 1e38).any()
    assert np.isfinite(scan.download()[0]).all()


def test_device_message_variant_equals_the_host_variant(capi, ctx, scan):
    import torch
    for name, pad in (("driver48", 0), ("step36_f64_at20", 4), ("step27_f64_at19", 3)):
        m, f, _ = Z.message(name, 1031, 5, seed=4, row_pad=pad)
        kt, kT = Z.knots(m, f, 64, seed=4)
        want = U.decode(m, f, kt, kT)
        stats, ustats = _counters(m, want)
        for shift in (0, 1):                                         # a device address that is not a multiple of 4
            d = torch.zeros(len(m.data) + 8, dtype=torch.uint8, device="cuda")
            d[shift:shift + len(m.data)] = torch.from_numpy(np.ascontiguousarray(m.data)).cuda()
            torch.cuda.synchronize()
            assert scan.decode_undistorted_device(m.layout(capi), d.data_ptr() + shift, len(m.data), f.capi(capi), kt, kT) == stats
            assert scan.undistort_stats() == ustats and _same(scan.download(), want)


def test_one_handle_alternating_plain_and_undistorted_decodes(capi, scan):
    """growing and shrinking messages and tracks on one handle: the running counters, the track's buffer and the plain
    decode's zeros"""
    seq = [("driver48", 37, 5, 3), ("step27_f32_at17", 1031, 7, 1025), ("step36_f64_at20", 4, 1, 1), ("step27_f64_at19", 640, 48, 64),
           ("driver48", 1024, 2, 65536), ("step27_f32_at17", 100, 1, 2)]
    for k, (name, w, h, K) in enumerate(seq):
        m, f, _ = Z.message(name, w, h, seed=10 + k, row_pad=k % 3)
        kt, kT = Z.knots(m, f, K, seed=10 + k)
        _check(capi, scan, m, f, kt, kT)
        _check_plain(capi, scan, m)
        _check(capi, scan, m, f, kt, kT)
    empty = S.Msg(0, 0, 48, S.FIELDS["driver48"])
    assert scan.decode_undistorted(empty.layout(capi), empty.data, capi.scan_time_field(0, 20, 1e-9), [0.0], [[1, 0, 0, 0, 0, 0, 0]]) == (0, 0)
    assert scan.undistort_stats() == (0, 0, 0) and scan.download()[0].shape == (0, 3)


def _refused(ctx, rc, code, text):
    msg = ctx.lib.vgx_last_error(ctx.h).decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_leave_the_scan_intact(capi, ctx, scan):
    m, f, _ = Z.message("step36_f64_at20", 211, 3, seed=5)
    kt, kT = Z.knots(m, f, 5, seed=5)
    want = _check(capi, scan, m, f, kt, kT)
    stats, ustats = _counters(m, want)
    lib, inv = ctx.lib, capi.ERR_INVALID
    data = np.ascontiguousarray(m.data)
    ptr, nb = C.c_void_p(data.ctypes.data), len(data)

    def decode(kt=kt, kT=kT, p=ptr, n_bytes=nb, device=False, null=None, n_knots=None, cfg=None, lay=None, **tf):
        d = dict(kind=f.kind, offset=f.offset, scale=f.scale, offset_s=f.offset_s)
        d.update(tf)
        field = capi.scan_time_field(**d)
        view, keep = capi.scan_track_view(kt, kT)
        if n_knots is not None:
            view.n_knots = n_knots
        layout = m.layout(capi)
        for k, v in (lay or {}).items():
            setattr(layout, k, v)
        fn = lib.vgx_scan_decode_msg_undistorted_device if device else lib.vgx_scan_decode_msg_undistorted
        return fn(scan.h, None if null == "layout" else C.byref(layout), None if cfg is None else C.byref(cfg),
                  None if null == "field" else C.byref(field), None if null == "track" else C.byref(view), p, n_bytes)

    bad_T = kT.copy()
    bad_T[3, 5] = np.inf
    name = "vgx_scan_decode_msg_undistorted: "
    cases = [
        (lambda: decode(null="layout"), name + "NULL layout"),
        (lambda: decode(null="field"), name + "NULL time field"),
        (lambda: decode(null="track"), name + "NULL track"),
        (lambda: decode(p=None), name + "NULL data"),
        (lambda: decode(p=None, device=True), "vgx_scan_decode_msg_undistorted_device: NULL data"),
        (lambda: decode(kind=7), "unknown time kind"),
        (lambda: decode(offset=29), "the time field does not fit in point_step"),
        (lambda: decode(kind=U.TIME_FLOAT32, offset=33), "the time field does not fit in point_step"),
        (lambda: decode(scale=np.nan), "the time field's scale or offset_s is not finite"),
        (lambda: decode(offset_s=-np.inf), "the time field's scale or offset_s is not finite"),
        (lambda: decode(n_knots=0), "n_knots is not in 1 .. 65536"),
        (lambda: decode(n_knots=65537), "n_knots is not in 1 .. 65536"),
        (lambda: decode(kt=[0.0, 0.1, 0.1, 0.2, 0.3]), "the knot times are not finite and strictly ascending"),
        (lambda: decode(kt=[0.0, 0.1, np.nan, 0.2, 0.3]), "the knot times are not finite and strictly ascending"),
        (lambda: decode(kT=bad_T), "a knot_T entry is not finite"),
        (lambda: decode(n_bytes=nb - 1), "n_bytes is less than (height - 1) * row_step + width * point_step"),
        (lambda: decode(lay=dict(offset_x=33)), "a coordinate field does not fit in point_step"),
        (lambda: decode(cfg=capi.scan_config(intensity_max=float("nan"))), "the intensity range is not finite or not max > min"),
    ]
    for call, text in cases:
        _refused(ctx, call(), inv, text)
        assert scan.stats() == stats and scan.undistort_stats() == ustats and _same(scan.download(), want), text
    _refused(ctx, decode(lay=dict(is_bigendian=1)), capi.ERR_UNSUPPORTED, "big-endian messages are not supported")
    assert lib.vgx_scan_undistort_stats(None, None, None, None) == inv
    assert lib.vgx_scan_decode_msg_undistorted(None, None, None, None, None, None, 0) == inv
    assert scan.stats() == stats and _same(scan.download(), want)


def _pose(k):
    return np.array([np.cos(0.05 * k), 0, 0, np.sin(0.05 * k), 0.1 + 0.15 * k, -0.05 * k, 0.02], F)


def _lidar_with_track(seed):
    """the 64 x 1024 driver48 LiDAR of the scan tests with column stamps in its t field and a knot every 16 columns"""
    m = S.lidar(seed, name="driver48")
    f = U.TimeField(U.TIME_UINT32, 20, 1e-9, 0.0)
    Z.put_time(m, f, np.tile(np.arange(1024, dtype=np.uint32) * np.uint32(97656), 64))
    kt, kT = Z.knots(m, f, 65, seed=seed)
    return m, f, kt, kT


def test_integrating_an_undistorted_scan_equals_integrating_the_restatements_arrays(capi, ctx, scan):
    cfg = capi.voxgraph_tsdf_config(deterministic=1)
    la, lb = capi.TsdfLayer(ctx, 0.2, 16), capi.TsdfLayer(ctx, 0.2, 16)
    ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
    for k in range(2):
        m, f, kt, kT = _lidar_with_track(40 + k)
        pts, rgba, _, st = U.decode(m, f, kt, kT)
        scan.decode_undistorted(m.layout(capi), m.data, f.capi(capi), kt, kT)
        na, nb = ia.integrate_scan(_pose(k), scan), ib.integratePointCloud(_pose(k), pts, rgba)
        assert na == nb > 0 and st["clamped"] > 0
    a, b = la.download(), lb.download()
    assert len(a[0]) > 5 and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    for o in (ia, ib, la, lb):
        o.destroy()


def test_registering_an_undistorted_scan_equals_registering_the_restatements_arrays(capi, ctx, scan):
    from tests import scan_registration_ref as G
    layer = capi.TsdfLayer(ctx, G.VOXEL_SIZE, G.VPS)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for k in range(3):
        integ.integratePointCloud(G.pose7(G.scan_pose(k)), G.room_scan(G.scan_pose(k)))
    m, f, kt, kT = _lidar_with_track(50)
    pts = U.decode(m, f, kt, kT)[0]
    scan.decode_undistorted(m.layout(capi), m.data, f.capi(capi), kt, kT)
    ra = capi.ScanRegistration(ctx, capi.scan_registration_config(G.MAX_ABS_DISTANCE))
    rb = capi.ScanRegistration(ctx, capi.scan_registration_config(G.MAX_ABS_DISTANCE))
    ra.set_points(scan)
    rb.set_points(pts)
    prior = G.pose7(G.seeded_prior(0))
    a, b = ra.evaluate(layer, prior, np.zeros(4)), rb.evaluate(layer, prior, np.zeros(4))
    flat = lambda r: np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in r])
    assert np.array_equal(flat(a).view(np.uint64), flat(b).view(np.uint64)) and np.abs(flat(a)).max() > 0
    for o in (ra, rb, integ, layer):
        o.destroy()
