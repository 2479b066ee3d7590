"""The scan decode without a GPU: hand-computed answers for the numpy restatement (tests/scan_msg_ref.py) that the GPU
tests compare the kernel with, the host-only entry points of the boundary (vgx_scan_layout_check,
vgx_scan_config_default) through ctypes, and the scenes' own invariants."""
import struct

import numpy as np
import pytest

from tests import scan_msg_ref as R
from tests import scan_msg_scenes as S

F = np.float32


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from voxgraph_amd import capi as m
    m.load()
    return m


def _f(v):
    return struct.pack("<f", v)


def test_known_bytes_xyzrgb():
    """pcl::PointXYZRGB, written out by hand: x y z pad | b g r a | pad; three points, the second has z = NaN"""
    pt = lambda x, y, z, rgb: _f(x) + _f(y) + z + b"\xee" * 4 + rgb + b"\xdd" * 12
    data = (pt(1.0, 2.0, b"\x00\x00\x00\x80", bytes([0x10, 0x20, 0x30, 0x40])) +           # z = -0.0
            pt(3.0, 4.0, b"\x00\x00\xc0\x7f", bytes([1, 2, 3, 4])) +                        # z = NaN
            pt(-5.5, 0.25, _f(7.0), bytes([0xff, 0x00, 0x80, 0x7f])))
    m = S.Msg(3, 1, 32, S.FIELDS["xyzrgb32"])
    m.data = np.frombuffer(data, np.uint8)
    p, c, kept = R.decode(m)
    assert kept.tolist() == [0, 2]
    assert p.view(np.uint32).tolist() == [[0x3f800000, 0x40000000, 0x80000000], [0xc0b00000, 0x3e800000, 0x40e00000]]
    assert c.tolist() == [[0x30, 0x20, 0x10, 0x40], [0x80, 0x00, 0xff, 0x7f]]       # (r, g, b, a) = (b2, b1, b0, b3)


def test_known_bytes_unaligned_step_and_row_padding():
    """point_step 7 (x, y, z overlapping at offsets 0, 1, 3), two rows of two points, 3 bytes of row padding: the
    addresses are r * row_step + c * point_step and nothing else"""
    row0 = bytes([0, 0, 0x80, 0x3f, 0, 0, 0x40]) + bytes([0, 0, 0x80, 0x7f, 0, 0, 0]) + b"\xaa\xbb\xcc"
    row1 = bytes([0, 0, 0, 0, 0, 0, 0]) + bytes([0x01, 0, 0, 0x80, 0, 0, 0xff]) + b"\x11\x22"      # (the last row's padding may be short)
    m = S.Msg(2, 2, 7, [("x", 0, S.FLOAT32, 1), ("y", 1, S.FLOAT32, 1), ("z", 3, S.FLOAT32, 1)], row_pad=3)
    m.data = np.frombuffer(row0 + row1, np.uint8)
    p, c, kept = R.decode(m, constant_rgba=(9, 8, 7, 6))
    # point 0: x = 3f800000, y = 003f8000, z = 4000003f; point 1: x = 7f800000 = +Inf: dropped; point 2: zeros
    # point 3: x = 80000001, y = 00800000, z = ff000080 (finite: exponent 0xfe)
    assert kept.tolist() == [0, 2, 3]
    assert p.view(np.uint32).tolist() == [[0x3f800000, 0x003f8000, 0x4000003f], [0, 0, 0], [0x80000001, 0x00800000, 0xff000080]]
    assert c.tolist() == [[9, 8, 7, 6]] * 3


def test_known_grey_levels():
    """grayColorMap over [0, 10000] (pointcloud_integrator.cpp:14): clamps with NaN -> min, h in f32, round half away"""
    v = np.array([5000, np.nan, -5, -0.0, 10000, 20000, np.inf, -np.inf, 39.0, 19.7, 19.5, 2530, 9990], F)
    #            127.5 -> 128          0       255    255    255      0     0.9945 0.50235 0.49725 64.515 254.745
    assert R.gray(v, 0, 10000).tolist() == [128, 0, 0, 0, 255, 255, 255, 0, 1, 1, 0, 65, 255]
    assert R.gray(np.array([15, 12, 10, 20, 9, np.nan], F), 10, 20).tolist() == [128, 51, 0, 255, 0, 0]
    m = S.Msg(2, 1, 32, S.FIELDS["xyzi32"])
    m.data = np.frombuffer((_f(1) + _f(2) + _f(3) + b"\x00" * 4 + _f(2530.0) + b"\x00" * 12) * 2, np.uint8)
    p, c, _ = R.decode(m)
    assert c.tolist() == [[65, 65, 65, 255]] * 2 and p.tolist() == [[1, 2, 3]] * 2


def test_scenes_hold_what_they_claim():
    for name, make in S.LAYOUTS.items():
        m = make()
        p, c, kept = R.decode(m)
        assert len(m.data) == m.height * m.row_step and len(p) == len(c) == len(kept) <= m.n
        assert np.isfinite(p).all() and np.all(np.diff(kept) > 0)
        if m.n > 100:
            assert 0 < len(kept) < m.n, name
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-1, 1, (185, 3)).astype(F)
    dropped = S.plant_specials(xyz)
    m = S.Msg(185, 1, 16, S.XYZ).fill(rng, xyz)
    p, _, kept = R.decode(m)
    assert sorted(set(range(185)) - set(kept.tolist())) == dropped and len(dropped) == 12
    assert np.array_equal(p.view(np.uint32), xyz[kept].view(np.uint32)) and (p.view(np.uint32) == 0x80000000).sum() == 3
    d = S.depth(0)
    _, _, kept = R.decode(d)
    assert 0.1 < 1 - len(kept) / d.n < 0.3                           # whole regions without depth
    i = S.small("xyzi32", 2)
    _, c, _ = R.decode(i)
    assert {0, 1, 128, 255} <= set(c[:, 0].tolist())                 # the planted intensities survive the filter


def test_config_defaults(capi):
    """pointcloud_integrator.cpp:12-14: a GrayscaleColorMap with setMaxValue(10000.0); a default voxblox::Color"""
    cfg = capi.scan_config()
    assert (cfg.intensity_min, cfg.intensity_max, list(cfg.constant_rgba)) == (0.0, 10000.0, [0, 0, 0, 0])
    assert (capi.SCAN_COLOR_NONE, capi.SCAN_COLOR_RGB, capi.SCAN_COLOR_INTENSITY) == (R.COLOR_NONE, R.COLOR_RGB, R.COLOR_INTENSITY)
    capi.load().vgx_scan_config_default(None)                        # NULL: nothing


def test_layout_check_accepts_and_refuses(capi):
    """vgx_scan_layout_check is host only: no device, no context"""
    ok, inv, uns = capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    for make in S.LAYOUTS.values():
        m = make()
        need = (m.height - 1) * m.row_step + m.width * m.point_step
        assert capi.scan_layout_check(m.layout(capi), len(m.data)) == ok
        assert capi.scan_layout_check(m.layout(capi), need) == ok              # the last row's padding need not exist
        assert capi.scan_layout_check(m.layout(capi), need - 1) == inv
    base = dict(width=10, height=4, point_step=16, offset_x=0, offset_y=4, offset_z=8)
    chk = lambda n_bytes=640, **kw: capi.scan_layout_check(capi.scan_layout(**{**base, **kw}), n_bytes)
    assert chk() == ok
    assert capi.scan_layout_check(None, 640) == inv
    assert chk(n_bytes=-1) == inv
    assert chk(point_step=0, row_step=0) == inv
    for f in ("offset_x", "offset_y", "offset_z"):
        assert chk(**{f: 12}) == ok and chk(**{f: 13}) == inv and chk(**{f: 0xfffffffe}) == inv
    assert chk(color_kind=capi.SCAN_COLOR_RGB, color_offset=12) == ok
    assert chk(color_kind=capi.SCAN_COLOR_INTENSITY, color_offset=13) == inv
    assert chk(color_kind=capi.SCAN_COLOR_NONE, color_offset=999) == ok          # not read
    assert chk(color_kind=3) == inv and chk(color_kind=-1) == inv
    assert chk(row_step=159) == inv and chk(row_step=160) == ok and chk(row_step=200, n_bytes=3 * 200 + 160) == ok
    assert chk(row_step=200, n_bytes=3 * 200 + 159) == inv
    assert chk(is_bigendian=1) == uns
    assert chk(width=0, n_bytes=0) == ok and chk(height=0, n_bytes=0) == ok      # empty clouds
    assert chk(point_step=1, offset_x=0, offset_y=0, offset_z=0) == inv          # 4 bytes do not fit in 1
    assert chk(point_step=4, offset_x=0, offset_y=0, offset_z=0, n_bytes=160) == ok
    # width * height >= 2^31: unsupported whatever n_bytes says; just below: a matter of n_bytes
    assert chk(width=1 << 16, height=1 << 15, row_step=16 << 16, n_bytes=1 << 40) == uns
    assert chk(width=(1 << 16) - 1, height=1 << 15, row_step=16 << 16, n_bytes=1 << 40) == ok
    assert chk(width=(1 << 16) - 1, height=1 << 15, row_step=16 << 16, n_bytes=1 << 30) == inv
    assert chk(width=0xffffffff, height=0xffffffff, point_step=0xffffffff, row_step=0xffffffff, n_bytes=1 << 62) == inv  # row_step < width * step
