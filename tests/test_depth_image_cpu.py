"""The depth-image decode's host side without a device: vgx_depth_image_check and vgx_depth_image_undistort_check (every
refusal of include/voxgraph_amd.h, "Depth-image scans", beside its accepted neighbour), the three structures' sizes against
the header's field lists, and the numpy restatement (tests/depth_image_ref.py) against the PointCloud2 restatement
(tests/scan_msg_ref.py): the unprojected candidates with NaN holes, decoded as a cloud, are the depth restatement's points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import depth_image_ref as D
from tests import scan_msg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    return m


def _check(capi, lay=None, cam=None, depth_n=None, color_n=None, **kw):
    """a 6 x 4 16UC1 image with an RGB8 colour image, rows padded by 2 and 1 bytes, with fields overridden"""
    l = dict(width=6, height=4, row_step=14, encoding=capi.DEPTH_16UC1, color_kind=capi.IMAGE_COLOR_RGB8, color_row_step=19)
    l.update(lay or {})
    c = dict(fx=5.0, fy=5.1, cx=2.7, cy=1.4)
    c.update(cam or {})
    layout, camera = capi.depth_image_layout(**l), capi.depth_camera(**c)
    bpp, cbpp = capi.DEPTH_BYTES_PER_PIXEL.get(layout.encoding, 2), capi.IMAGE_COLOR_BYTES_PER_PIXEL.get(layout.color_kind, 3)
    need = (layout.height - 1) * layout.row_step + layout.width * bpp if layout.width * layout.height else 0
    cneed = (layout.height - 1) * layout.color_row_step + layout.width * cbpp if layout.width * layout.height else 0
    return capi.depth_image_check(layout, camera, need if depth_n is None else need + depth_n, cneed if color_n is None else cneed + color_n,
                                  **kw)


def test_check_refusals_and_their_accepted_neighbours(capi):
    ok, inv, uns = capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    nan, inf = float("nan"), float("inf")
    assert _check(capi) == ok
    cam = capi.depth_camera(fx=1.0, fy=1.0)
    assert capi.depth_image_check(None, cam, 0) == inv and capi.depth_image_check(capi.depth_image_layout(), None, 0) == inv
    assert capi.depth_image_check(capi.depth_image_layout(), cam, 0) == ok                # (an empty image, no bytes)
    # encodings and colour kinds
    assert _check(capi, lay=dict(encoding=2)) == inv and _check(capi, lay=dict(encoding=-1)) == inv
    assert _check(capi, lay=dict(encoding=capi.DEPTH_32FC1, row_step=24)) == ok
    assert _check(capi, lay=dict(color_kind=6)) == inv and _check(capi, lay=dict(color_kind=-1)) == inv
    for kind, step in ((capi.IMAGE_COLOR_NONE, 0), (capi.IMAGE_COLOR_BGR8, 18), (capi.IMAGE_COLOR_RGBA8, 24), (capi.IMAGE_COLOR_BGRA8, 24),
                       (capi.IMAGE_COLOR_MONO8, 6)):
        assert _check(capi, lay=dict(color_kind=kind, color_row_step=step)) == ok
        if step:
            assert _check(capi, lay=dict(color_kind=kind, color_row_step=step - 1)) == inv
    # row steps: width * bytes per pixel is the least
    assert _check(capi, lay=dict(row_step=12)) == ok and _check(capi, lay=dict(row_step=11)) == inv
    assert _check(capi, lay=dict(row_step=13)) == ok                                      # (odd: legal)
    assert _check(capi, lay=dict(encoding=capi.DEPTH_32FC1, row_step=23)) == inv
    assert _check(capi, lay=dict(color_row_step=18)) == ok and _check(capi, lay=dict(color_row_step=17)) == inv
    # byte counts: one short of (height - 1) * row_step + width * bytes per pixel; negative
    assert _check(capi, depth_n=-1) == inv and _check(capi, depth_n=0) == ok and _check(capi, depth_n=5) == ok
    assert _check(capi, color_n=-1) == inv and _check(capi, color_n=0) == ok
    assert _check(capi, lay=dict(color_kind=capi.IMAGE_COLOR_NONE), color_n=-1000) == ok  # (not read)
    assert _check(capi, depth_n=-1000) == inv
    assert _check(capi, lay=dict(width=0), depth_n=0, color_n=0) == ok and _check(capi, lay=dict(height=0)) == ok
    # the camera
    for k in ("fx", "fy"):
        for bad in (0.0, -0.0, nan, inf, -inf):
            assert _check(capi, cam={k: bad}) == inv, (k, bad)
        assert _check(capi, cam={k: -3.0}) == ok and _check(capi, cam={k: 1e-300}) == ok
    for k in ("cx", "cy"):
        for bad in (nan, inf, -inf):
            assert _check(capi, cam={k: bad}) == inv, (k, bad)
        assert _check(capi, cam={k: -1e9}) == ok
    for bad in (0.0, -0.001, nan, inf):
        assert _check(capi, cam=dict(depth_unit_m=bad)) == inv, bad
        assert _check(capi, lay=dict(encoding=capi.DEPTH_32FC1, row_step=24), cam=dict(depth_unit_m=bad)) == ok   # (not read)
    assert _check(capi, cam=dict(depth_unit_m=1e-45)) == ok
    assert _check(capi, cam=dict(min_depth_m=nan)) == inv and _check(capi, cam=dict(max_depth_m=nan)) == inv
    assert _check(capi, cam=dict(min_depth_m=-1e-30)) == inv and _check(capi, cam=dict(min_depth_m=0.0)) == ok
    assert _check(capi, cam=dict(min_depth_m=2.0, max_depth_m=2.0)) == ok                 # (min == max)
    assert _check(capi, cam=dict(min_depth_m=2.0, max_depth_m=float(np.nextafter(F(2), F(0))))) == inv
    assert _check(capi, cam=dict(min_depth_m=inf, max_depth_m=inf)) == ok
    for k in ("stride_u", "stride_v"):
        assert _check(capi, cam={k: 0}) == inv and _check(capi, cam={k: -1}) == inv
        assert _check(capi, cam={k: 1}) == ok and _check(capi, cam={k: 1000}) == ok
    # unsupported
    assert _check(capi, lay=dict(is_bigendian=1)) == uns and _check(capi, lay=dict(is_bigendian=0)) == ok
    big = capi.depth_image_layout(width=1 << 16, height=1 << 15, encoding=capi.DEPTH_16UC1)
    assert capi.depth_image_check(big, cam, 1 << 40) == uns
    big.height -= 1
    assert capi.depth_image_check(big, cam, 1 << 40) == ok and capi.depth_image_check(big, cam, big.height * big.row_step - 1) == inv


def test_undistort_check_refusals_and_their_accepted_neighbours(capi):
    ok, inv = capi.OK, capi.ERR_INVALID
    nan, inf = float("nan"), float("inf")
    I7 = [1, 0, 0, 0, 0, 0, 0]
    rt = capi.depth_row_time(1e-4, 0.01)
    assert _check(capi, row_time=rt, knot_time=[0.0, 0.1], knot_T=[I7, I7]) == ok
    assert _check(capi, row_time=None, knot_time=[0.0], knot_T=[I7]) == inv               # NULL row time
    assert _check(capi, row_time=rt) == inv                                               # NULL track
    for bad in (nan, inf, -inf):
        assert _check(capi, row_time=capi.depth_row_time(bad, 0.0), knot_time=[0.0], knot_T=[I7]) == inv
        assert _check(capi, row_time=capi.depth_row_time(0.0, bad), knot_time=[0.0], knot_T=[I7]) == inv
    assert _check(capi, row_time=capi.depth_row_time(0.0, 0.0), knot_time=[0.0], knot_T=[I7]) == ok
    assert _check(capi, row_time=capi.depth_row_time(-1e300, 1e300), knot_time=[0.0], knot_T=[I7]) == ok
    # the track: what vgx_scan_undistort_check refuses
    assert _check(capi, row_time=rt, knot_time=[], knot_T=np.zeros((0, 7))) == inv
    assert _check(capi, row_time=rt, knot_time=[0.0, 0.0], knot_T=[I7, I7]) == inv
    assert _check(capi, row_time=rt, knot_time=[0.1, 0.0], knot_T=[I7, I7]) == inv
    assert _check(capi, row_time=rt, knot_time=[0.0, nan], knot_T=[I7, I7]) == inv
    assert _check(capi, row_time=rt, knot_time=[0.0, 0.1], knot_T=[I7, [1, 0, 0, 0, inf, 0, 0]]) == inv
    assert _check(capi, row_time=rt, knot_time=np.arange(65537.0), knot_T=np.tile(I7, (65537, 1))) == inv
    assert _check(capi, row_time=rt, knot_time=np.arange(65536.0), knot_T=np.tile(I7, (65536, 1))) == ok
    # and everything the plain check refuses
    assert _check(capi, lay=dict(row_step=11), row_time=rt, knot_time=[0.0], knot_T=[I7]) == inv
    assert _check(capi, depth_n=-1, row_time=rt, knot_time=[0.0], knot_T=[I7]) == inv
    assert _check(capi, lay=dict(is_bigendian=1), row_time=rt, knot_time=[0.0], knot_T=[I7]) == capi.ERR_UNSUPPORTED


def test_checks_need_no_context(capi):
    """the library's handles are never made: the check is arithmetic on its arguments"""
    lib = capi.load()
    lay, cam = capi.depth_image_layout(width=3, height=2, encoding=capi.DEPTH_32FC1), capi.depth_camera(fx=2.0, fy=2.0)
    assert lib.vgx_depth_image_check(C.byref(lay), C.byref(cam), 24, 0) == capi.OK
    assert lib.vgx_depth_image_check(C.byref(lay), C.byref(cam), 23, 0) == capi.ERR_INVALID
    assert lib.vgx_depth_image_check(None, None, 0, 0) == capi.ERR_INVALID


def test_camera_defaults(capi):
    cam = capi.depth_camera()
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (0.0, 0.0, 0.0, 0.0) and cam.depth_unit_m == F(0.001)
    assert cam.min_depth_m == 0.0 and cam.max_depth_m == float("inf") and (cam.stride_u, cam.stride_v) == (1, 1)
    capi.load().vgx_depth_camera_default(None)


C_TYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}


def _header_struct(name):
    """a ctypes.Structure from the field list of `typedef struct name { ... } name;` in the header"""
    text = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(",")]
    return type(name, (C.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("name,cls", [("vgx_depth_image_layout", "DepthImageLayout"), ("vgx_depth_camera", "DepthCamera"),
                                      ("vgx_depth_row_time", "DepthRowTime")])
def test_structures_match_the_header(capi, name, cls):
    want, got = _header_struct(name), getattr(capi, cls)
    assert C.sizeof(got) == C.sizeof(want) and [f[0] for f in got._fields_] == [f[0] for f in want._fields_]
    assert all(getattr(got, f[0]).offset == getattr(want, f[0]).offset for f in want._fields_)
    assert C.sizeof(got) == {"vgx_depth_image_layout": 28, "vgx_depth_camera": 56, "vgx_depth_row_time": 16}[name]


@pytest.mark.parametrize("encoding", [D.DEPTH_16UC1, D.DEPTH_32FC1])
@pytest.mark.parametrize("width,height,su,sv,pad", [(41, 25, 1, 1, 0), (41, 25, 2, 3, 5), (7, 5, 1, 1, 1), (1, 1, 1, 1, 0), (64, 3, 5, 1, 3)])
def test_restatement_equals_the_cloud_restatement_on_its_unprojected_points(encoding, width, height, su, sv, pad):
    """gate open and no overflow: the depth restatement's dropped candidates are exactly its invalid ones, so a cloud that
    holds NaN there and the unprojected point elsewhere decodes to the same points in the same order"""
    img = D.planted_image(width, height, encoding, seed=width + su, row_pad=pad)
    if encoding == D.DEPTH_32FC1:                                                         # (3e38 would overflow x: not here)
        z = img.depth.reshape(height, -1)[:, :4 * width].copy().view(F)
        z[z == F(3e38)] = F(3.0)
        img = D.Image(width, height, encoding, D.rows(z, pad, 0xAB)[0], img.row_step)
    cam = D.camera_for(width, height, stride_u=su, stride_v=sv)
    pts, reason, u, v = D.unproject(img, cam)
    want = D.decode(img, cam, constant_rgba=(9, 8, 7, 6))
    assert set(np.unique(reason)) <= {0, 1} and want[3]["candidates"] == len(u) == -(-width // su) * -(-height // sv)
    m = D.as_cloud(img, cam, pts)
    got = R.decode(m, constant_rgba=(9, 8, 7, 6))
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and len(got[2]) + want[3]["invalid"] == len(u)
    if width * height >= 35:
        assert want[3]["invalid"] > 0 and len(want[2]) > 0
    # the points are the pinhole model's: u = fx x / z + cx within rounding (a denormal depth has no precision to speak of)
    p = want[0][want[0][:, 2] > 1e-3].astype(np.float64)
    k = want[2][want[0][:, 2] > 1e-3]
    assert np.allclose(p[:, 0] / p[:, 2] * cam.fx + cam.cx, u[k], atol=1e-3)
    assert np.allclose(p[:, 1] / p[:, 2] * cam.fy + cam.cy, v[k], atol=1e-3)


def test_restatement_counts_each_reason_once_and_in_order():
    """one row of planted depths whose fate is known: invalid before the gate, the gate before the overflow"""
    z = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-40, 3e38, 0.25, 8.0, 0.2499, 8.001, 3.0, 1e-40], F).reshape(1, -1)
    img = D.Image(14, 1, D.DEPTH_32FC1, z.tobytes())
    shut = D.decode(img, D.Camera(10.0, 10.0, 0.5, 0.0, min_depth_m=0.25, max_depth_m=8.0))
    assert shut[3] == dict(candidates=14, invalid=6, out_of_range=5, overflowed=0, bad_time=0, track_overflowed=0, clamped=0)
    assert list(shut[2]) == [8, 9, 12]
    opened = D.decode(img, D.Camera(10.0, 10.0, 0.5, 0.0))
    assert opened[3]["invalid"] == 6 and opened[3]["out_of_range"] == 0 and opened[3]["overflowed"] == 1
    assert list(opened[2]) == [6, 8, 9, 10, 11, 12, 13] and D.dropped(opened[3]) == 7
    assert opened[0][0, 2] == F(1e-40) and opened[0][0, 0] != 0                            # (a denormal depth is a depth)
    raw = np.array([[0, 1, 65535, 250, 8000, 8001]], np.uint16)
    got = D.decode(D.Image(6, 1, D.DEPTH_16UC1, raw.tobytes()), D.Camera(10.0, 10.0, 0.5, 0.0, min_depth_m=0.25, max_depth_m=8.0))
    assert got[3]["invalid"] == 1 and list(got[2]) == [3, 4] and got[3]["out_of_range"] == 3
