"""A raw sensor_msgs/PointCloud2 decoded on the device (vgx_scan, voxgraph_amd/csrc/vgx_scan.hip) against its numpy
restatement (tests/scan_msg_ref.py), bit for bit: points as uint32, colours, count and order; and the layers the
integrators build from a decoded scan against the layers they build from the restatement's arrays."""
import ctypes as C

import numpy as np
import pytest

from tests import scan_msg_ref as R
from tests import scan_msg_scenes as S

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
    (gp, gc), (wp, wc, _) = got, want
    return (gp.shape == wp.shape and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)) and gc.shape == wc.shape
            and np.array_equal(gc, wc))


def _check_decode(capi, scan, m, **cfg):
    want = R.decode(m, **{k: v for k, v in cfg.items()})
    n, dropped = scan.decode_msg(m.layout(capi), m.data, capi.scan_config(**cfg) if cfg else None)
    assert (n, dropped) == (len(want[0]), m.n - len(want[0])) and scan.stats() == (n, dropped)
    assert _same(scan.download(), want)
    return want


@pytest.mark.parametrize("name", list(S.LAYOUTS))
def test_decode_equals_the_restatement(capi, scan, name):
    m = S.LAYOUTS[name]()
    _check_decode(capi, scan, m)
    # another grey range and another constant colour, on the same handle
    _check_decode(capi, scan, m, intensity_min=-50.0, intensity_max=7000.0, constant_rgba=(1, 2, 3, 254))


def _pose(k):
    return np.array([np.cos(0.05 * k), 0, 0, np.sin(0.05 * k), 0.1 + 0.15 * k, -0.05 * k, 0.02], F)


def _layers_identical(a, b):
    """block order included, every array as bytes"""
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["reproducible_mixed", "reproducible_sorted", "merged"])
def test_integrating_a_raw_message_equals_integrating_the_restatements_arrays(capi, ctx, scan, mode):
    order = capi.TSDF_ORDER_SORTED if mode == "reproducible_sorted" else capi.TSDF_ORDER_MIXED
    cfg = capi.voxgraph_tsdf_config(deterministic=1, integration_order=order)
    merged = mode == "merged"
    for scene in (S.lidar, S.depth):
        la, lb = capi.TsdfLayer(ctx, 0.2, 16), capi.TsdfLayer(ctx, 0.2, 16)
        ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
        for k in range(3):
            m = scene(10 + k)
            pts, rgba, _ = R.decode(m)
            scan.decode_msg(m.layout(capi), m.data)
            if merged:
                na, nb = ia.integrate_merged_scan(_pose(k), scan), ib.integratePointCloudMerged(_pose(k), pts, rgba)
            else:
                na, nb = ia.integrate_scan(_pose(k), scan), ib.integratePointCloud(_pose(k), pts, rgba)
            assert na == nb > 0, (scene.__name__, k, na, nb)
        a, b = la.download(), lb.download()
        assert len(a[0]) > 5 and _layers_identical(a, b), (scene.__name__, len(a[0]), len(b[0]))
        for o in (ia, ib, la, lb):
            o.destroy()


def _sorted_blocks(layer):
    bi, d, w, rgba = layer.download()
    o = np.lexsort((bi[:, 2], bi[:, 1], bi[:, 0]))
    return bi[o], d[o], w[o], rgba[o]


def test_racing_mode_on_an_order_independent_scan(capi, ctx, scan):
    """carving off and end points 1.3 m apart with a 0.25 m truncation: no two rays share a voxel, so the racing
    integrator has one legal result; only the order blocks are allocated in is free"""
    cfg = capi.tsdf_config(default_truncation_distance=0.25, voxel_carving_enabled=0, use_const_weight=0, max_ray_length_m=30.0)
    la, lb = capi.TsdfLayer(ctx, 0.1, 16), capi.TsdfLayer(ctx, 0.1, 16)
    ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
    T = np.array([1, 0, 0, 0, 0.07, -0.03, 0.02], F)
    for k in range(2):
        m = S.lattice(k)
        pts, rgba, kept = R.decode(m)
        assert 0 < len(kept) < m.n
        scan.decode_msg(m.layout(capi), m.data)
        na, nb = ia.integrate_scan(T, scan), ib.integratePointCloud(T, pts, rgba)
        assert na == nb > 100
    assert _layers_identical(_sorted_blocks(la), _sorted_blocks(lb))
    for o in (ia, ib, la, lb):
        o.destroy()


def test_a_cloud_with_nan_returns_touches_the_blocks_its_filtered_arrays_touch(capi, ctx, scan):
    """the integrators let a NaN point through isPointValid, as voxblox does: the decode is what keeps such returns
    out.  Racing mode with what makes its SET of updated voxels independent of the order: one point per start cell,
    the early-out disabled, constant weights (weight = number of rays through the voxel, an integer sum)."""
    vs = 0.1
    cfg = capi.tsdf_config(default_truncation_distance=0.3, max_ray_length_m=20.0, use_const_weight=1, use_weight_dropoff=0,
                           max_consecutive_ray_collisions=1 << 30)
    m = S.lidar(5, rows=24, cols=360)
    xyz, _, kept = R.decode(m)
    cells = np.floor(xyz * F(2.0 / vs) + 1e-6).astype(np.int64)
    _, first = np.unique(cells, axis=0, return_index=True)
    dup = np.setdiff1d(np.arange(len(xyz)), first)           # a second point in a start cell: made a NaN return too
    rng = np.random.default_rng(1)
    full = np.full((m.n, 3), np.nan, F)
    full[kept] = xyz
    full[kept[dup]] = np.nan
    m.fill(rng, full, rng.uniform(0, 10000, m.n).astype(F))
    pts, rgba, kept2 = R.decode(m)
    assert 2000 < len(kept2) < m.n - 200
    la, lb = capi.TsdfLayer(ctx, vs, 16), capi.TsdfLayer(ctx, vs, 16)
    ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
    T = np.array([1, 0, 0, 0, 0, 0, 0], F)
    n, dropped = scan.decode_msg(m.layout(capi), m.data)
    assert (n, dropped) == (len(pts), m.n - len(pts))
    na, nb = ia.integrate_scan(T, scan), ib.integratePointCloud(T, pts, rgba)
    assert na == nb > 10000
    a, b = _sorted_blocks(la), _sorted_blocks(lb)
    assert np.array_equal(a[0], b[0]) and len(a[0]) > 20             # exactly the same blocks
    assert np.array_equal(a[2], b[2])                                # and the same number of rays through every voxel
    for o in (ia, ib, la, lb):
        o.destroy()


def _refused(ctx, rc, code, text):
    msg = ctx.lib.vgx_last_error(ctx.h).decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_leave_the_scan_intact(capi, ctx, scan):
    m = S.small("xyzi32", 2)
    want = _check_decode(capi, scan, m)
    lib, inv, uns = ctx.lib, capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    data = np.ascontiguousarray(m.data)
    ptr, nb = C.c_void_p(data.ctypes.data), len(data)

    def decode(n_bytes=nb, p=ptr, cfg=None, device=False, **kw):
        lay = m.layout(capi)
        for k, v in kw.items():
            setattr(lay, k, v)
        fn = lib.vgx_scan_decode_msg_device if device else lib.vgx_scan_decode_msg
        return fn(scan.h, C.byref(lay), None if cfg is None else C.byref(cfg), p, n_bytes)

    need = (m.height - 1) * m.row_step + m.width * m.point_step
    cases = [
        (lambda: lib.vgx_scan_decode_msg(scan.h, None, None, ptr, nb), inv, "vgx_scan_decode_msg: NULL layout"),
        (lambda: decode(p=None), inv, "vgx_scan_decode_msg: NULL data"),
        (lambda: decode(p=None, device=True), inv, "vgx_scan_decode_msg_device: NULL data"),
        (lambda: decode(n_bytes=-1), inv, "n_bytes is negative"),
        (lambda: decode(point_step=0), inv, "point_step is 0"),
        (lambda: decode(offset_x=29), inv, "a coordinate field does not fit in point_step"),
        (lambda: decode(offset_y=30), inv, "a coordinate field does not fit in point_step"),
        (lambda: decode(offset_z=0xffffffff), inv, "a coordinate field does not fit in point_step"),
        (lambda: decode(color_offset=29), inv, "the colour field does not fit in point_step"),
        (lambda: decode(row_step=m.width * m.point_step - 1), inv, "row_step is less than width * point_step"),
        (lambda: decode(n_bytes=need - 1), inv, "n_bytes is less than (height - 1) * row_step + width * point_step"),
        (lambda: decode(color_kind=3), inv, "unknown color_kind"),
        (lambda: decode(cfg=capi.scan_config(intensity_max=float("nan"))), inv, "the intensity range is not finite or not max > min"),
        (lambda: decode(cfg=capi.scan_config(intensity_min=float("-inf"))), inv, "the intensity range is not finite or not max > min"),
        (lambda: decode(cfg=capi.scan_config(intensity_min=5.0, intensity_max=5.0)), inv, "the intensity range is not finite or not max > min"),
        (lambda: decode(is_bigendian=1), uns, "big-endian messages are not supported"),
        (lambda: decode(width=1 << 16, height=1 << 15, row_step=32 << 16, n_bytes=1 << 40), uns, "width * height is 2^31 or more"),
    ]
    for call, code, text in cases:
        _refused(ctx, call(), code, text)
        assert scan.stats() == (len(want[0]), m.n - len(want[0])) and _same(scan.download(), want), text
    assert lib.vgx_scan_decode_msg(None, C.byref(m.layout(capi)), None, ptr, nb) == inv
    assert lib.vgx_scan_stats(None, None, None) == inv and lib.vgx_scan_destroy(None) == inv
    assert lib.vgx_scan_download(None, None, None) == inv and lib.vgx_scan_device_pointers(None, None, None) == inv
    _refused(ctx, lib.vgx_scan_create(ctx.h, None), inv, "vgx_scan_create: NULL argument")
    # the integrate entry points: NULL handles, a scan of another context
    layer = capi.TsdfLayer(ctx, 0.2, 16)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(), layer)
    T = np.array([1, 0, 0, 0, 0, 0, 0], F)
    Tp = T.ctypes.data_as(capi.f32p)
    for fn, name in ((lib.vgx_tsdf_integrate_scan, "vgx_tsdf_integrate_scan"), (lib.vgx_tsdf_integrate_merged_scan, "vgx_tsdf_integrate_merged_scan")):
        _refused(ctx, fn(integ.h, Tp, None, 0, None), inv, name + ": NULL argument")
        _refused(ctx, fn(integ.h, None, scan.h, 0, None), inv, name + ": NULL argument")
        assert fn(None, Tp, scan.h, 0, None) == inv
        other = capi.Context(0)
        foreign = capi.Scan(other)
        _refused(ctx, fn(integ.h, Tp, foreign.h, 0, None), inv, name + ": the scan belongs to another context")
        foreign.destroy()
        other.close()
    assert layer.stats()[0] == 0 and _same(scan.download(), want)
    integ.destroy()
    layer.destroy()


def test_empty_and_all_dropped_clouds(capi, ctx, scan):
    layer = capi.TsdfLayer(ctx, 0.2, 16)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    T = np.array([1, 0, 0, 0, 0, 0, 0], F)
    _check_decode(capi, scan, S.small("xyzrgb32", 3))                 # the handle holds a scan: the empty ones replace it
    empties = [S.Msg(0, 0, 16, S.XYZ), S.Msg(0, 7, 32, S.FIELDS["xyzi32"]), S.Msg(9, 0, 32, S.FIELDS["xyzrgb32"], row_pad=4)]
    rng = np.random.default_rng(0)
    for bad in (np.nan, np.inf):
        for name in ("xyz16", "unaligned19_rgb"):
            xyz = rng.uniform(-1, 1, (3000, 3)).astype(F)
            xyz[np.arange(3000), rng.integers(0, 3, 3000)] = bad
            empties.append(S.Msg(1000, 3, S.STEP[name], S.FIELDS[name]).fill(rng, xyz, rng.integers(0, 255, 3000).astype(np.uint32)))
    for m in empties:
        assert scan.decode_msg(m.layout(capi), m.data) == (0, m.n)
        pts, rgba = scan.download()
        assert pts.shape == (0, 3) and rgba.shape == (0, 4) and scan.device_pointers() == (None, None)
        assert integ.integrate_scan(T, scan) == 0 and integ.integrate_merged_scan(T, scan) == 0
        assert integ.integrate_scan(T, scan, count=False) == 0
        _check_decode(capi, scan, S.small("xyz16", 1))
    assert layer.stats() == (0, 0)
    integ.destroy()
    layer.destroy()


def test_one_handle_over_growing_and_shrinking_messages(capi, ctx, scan):
    for make in (lambda: S.small("xyz16", 1), lambda: S.depth(3), lambda: S.small("unaligned19_rgb", 5), lambda: S.lidar(3),
                 lambda: S.depth(4, row_pad=12), lambda: S.small("driver48", 4, width=2048, height=3), lambda: S.Msg(0, 0, 16, S.XYZ),
                 lambda: S.lidar(4, name="driver48")):
        _check_decode(capi, scan, make())
    # decoding again right after an uncounted integrate: both are on the TSDF stream, the queued scan reads first
    cfg = capi.voxgraph_tsdf_config(deterministic=1)
    la, lb = capi.TsdfLayer(ctx, 0.2, 16), capi.TsdfLayer(ctx, 0.2, 16)
    ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
    msgs = [S.lidar(20), S.depth(21), S.lidar(22, rows=16, cols=512), S.lidar(23)]
    for k, m in enumerate(msgs):
        scan.decode_msg(m.layout(capi), m.data)
        assert ia.integrate_scan(_pose(k), scan, count=False) == 0
    for k, m in enumerate(msgs):
        pts, rgba, _ = R.decode(m)
        ib.integratePointCloud(_pose(k), pts, rgba, count=False)
    assert _layers_identical(la.download(), lb.download()) and la.stats()[0] > 5
    for o in (ia, ib, la, lb):
        o.destroy()


def test_device_pointer_variant_equals_the_host_variant(capi, ctx, scan):
    import torch
    other = capi.Scan(ctx)
    for name in ("xyzi32", "unaligned19_intensity", "padded_rows_unaligned", "depth_480x640", "lidar_driver48"):
        m = S.LAYOUTS[name]()
        want = _check_decode(capi, scan, m)
        for shift in (0, 1):                                         # a device address that is not a multiple of 4
            d = torch.zeros(len(m.data) + 8, dtype=torch.uint8, device="cuda")
            d[shift:shift + len(m.data)] = torch.from_numpy(np.ascontiguousarray(m.data)).cuda()
            torch.cuda.synchronize()
            assert other.decode_msg_device(m.layout(capi), d.data_ptr() + shift, len(m.data)) == (len(want[0]), m.n - len(want[0]))
            assert _same(other.download(), want)
    # the arrays behind vgx_scan_device_pointers are the scan: integrating them is integrating the scan
    n = other.stats()[0]
    p = other.device_pointers()
    assert n > 0 and p[0] and p[1]
    cfg = capi.voxgraph_tsdf_config(deterministic=1)
    la, lb = capi.TsdfLayer(ctx, 0.2, 16), capi.TsdfLayer(ctx, 0.2, 16)
    ia, ib = capi.FastTsdfIntegrator(ctx, cfg, la), capi.FastTsdfIntegrator(ctx, cfg, lb)
    assert ia.integrate_scan(_pose(0), other) == ib.integrate_device(_pose(0), p[0], p[1], n, count=True) > 10000
    assert _layers_identical(la.download(), lb.download())
    for o in (ia, ib, la, lb):
        o.destroy()
    other.destroy()
