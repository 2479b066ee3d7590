"""numpy restatement of the depth-image decode (include/voxgraph_amd.h, "Depth-image scans").  Written from the rules in the
header, not from the kernel: candidates from the strides, depths assembled byte by byte, the four filter steps in their
order with one counter each, the unprojection in f32 one rounding per operation with the host's f64 -> f32 constants, the
track step of tests/scan_undistort_ref.py on the row time, colours from the colour image's bytes.  numpy never contracts a
multiply and an add.  Below the restatement: the builders the tests make their images with."""
import numpy as np

from tests import scan_msg_ref as R
from tests import scan_undistort_ref as U

F = np.float32
DEPTH_16UC1, DEPTH_32FC1 = 0, 1
COLOR_NONE, COLOR_RGB8, COLOR_BGR8, COLOR_RGBA8, COLOR_BGRA8, COLOR_MONO8 = 0, 1, 2, 3, 4, 5
DEPTH_BPP = {DEPTH_16UC1: 2, DEPTH_32FC1: 4}
COLOR_BPP = {COLOR_NONE: 0, COLOR_RGB8: 3, COLOR_BGR8: 3, COLOR_RGBA8: 4, COLOR_BGRA8: 4, COLOR_MONO8: 1}


class Image:
    """a depth image's bytes and header, with its registered colour image's"""

    def __init__(self, width, height, encoding, depth, row_step=None, color_kind=COLOR_NONE, color=None, color_row_step=None):
        self.width, self.height, self.encoding, self.color_kind = int(width), int(height), encoding, color_kind
        self.row_step = self.width * DEPTH_BPP[encoding] if row_step is None else int(row_step)
        self.color_row_step = self.width * COLOR_BPP[color_kind] if color_row_step is None else int(color_row_step)
        self.depth = np.ascontiguousarray(np.frombuffer(depth, np.uint8))
        self.color = None if color is None else np.ascontiguousarray(np.frombuffer(color, np.uint8))

    def layout(self, capi, **kw):
        d = dict(width=self.width, height=self.height, row_step=self.row_step, encoding=self.encoding, color_kind=self.color_kind,
                 color_row_step=self.color_row_step)
        d.update(kw)
        return capi.depth_image_layout(**d)


class Camera:
    def __init__(self, fx, fy, cx, cy, depth_unit_m=0.001, min_depth_m=0.0, max_depth_m=np.inf, stride_u=1, stride_v=1):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.depth_unit_m, self.min_depth_m, self.max_depth_m = depth_unit_m, min_depth_m, max_depth_m
        self.stride_u, self.stride_v = int(stride_u), int(stride_v)

    def capi(self, capi, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return capi.depth_camera(**d)


def candidates(img, cam):
    """(u, v) of every candidate in ascending candidate index: int64 arrays of wc * hc entries"""
    us, vs = np.arange(0, img.width, cam.stride_u, dtype=np.int64), np.arange(0, img.height, cam.stride_v, dtype=np.int64)
    v, u = np.meshgrid(vs, us, indexing="ij")
    return u.reshape(-1), v.reshape(-1)


def depths(img, cam, u, v):
    """z of the pixels (u, v): f32"""
    data = img.depth
    if img.encoding == DEPTH_16UC1:
        at = v * np.int64(img.row_step) + 2 * u
        raw = data[at].astype(np.uint32) | (data[at + 1].astype(np.uint32) << np.uint32(8))
        return (raw.astype(F) * F(cam.depth_unit_m)).astype(F)
    if img.encoding == DEPTH_32FC1:
        return R.field_u32(data, v * np.int64(img.row_step) + 4 * u, 0).view(F)
    raise ValueError("unknown encoding")


def unproject(img, cam):
    """Filter steps 1 to 4 on every candidate -> (points [n_candidates][3] f32, reason [n_candidates] uint8, u, v) with
    reason 0 kept, 1 invalid, 2 out of range, 3 overflowed; the points of dropped candidates are NaN"""
    u, v = candidates(img, cam)
    pts = np.full((len(u), 3), np.nan, F)
    reason = np.zeros(len(u), np.uint8)
    if len(u) == 0:
        return pts, reason, u, v
    z = depths(img, cam, u, v)
    cxf, cyf, kx, ky = F(cam.cx), F(cam.cy), F(1.0 / cam.fx), F(1.0 / cam.fy)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (F(0) < z) & (z < F(np.inf))
        in_range = (F(cam.min_depth_m) <= z) & (z <= F(cam.max_depth_m))
        x = (((u.astype(F) - cxf).astype(F) * z).astype(F) * kx).astype(F)
        y = (((v.astype(F) - cyf).astype(F) * z).astype(F) * ky).astype(F)
    finite = np.isfinite(x) & np.isfinite(y)
    reason[valid & in_range & ~finite] = 3
    reason[valid & ~in_range] = 2
    reason[~valid] = 1
    k = reason == 0
    pts[k, 0], pts[k, 1], pts[k, 2] = x[k], y[k], z[k]
    return pts, reason, u, v


def colours(img, u, v, constant_rgba=(0, 0, 0, 0)):
    """rgba [n][4] u8 of the pixels (u, v)"""
    rgba = np.zeros((len(u), 4), np.uint8)
    kind = img.color_kind
    if kind == COLOR_NONE:
        rgba[:] = np.asarray(constant_rgba, np.uint8)
        return rgba
    at = v * np.int64(img.color_row_step) + u * COLOR_BPP[kind]
    b = [img.color[at + k] for k in range(COLOR_BPP[kind])]
    if kind == COLOR_MONO8:
        r, g, bl, a = b[0], b[0], b[0], 255
    elif kind in (COLOR_RGB8, COLOR_RGBA8):
        r, g, bl, a = b[0], b[1], b[2], (b[3] if kind == COLOR_RGBA8 else 255)
    elif kind in (COLOR_BGR8, COLOR_BGRA8):
        r, g, bl, a = b[2], b[1], b[0], (b[3] if kind == COLOR_BGRA8 else 255)
    else:
        raise ValueError("unknown color_kind")
    rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3] = r, g, bl, a
    return rgba


def decode(img, cam, constant_rgba=(0, 0, 0, 0), row_time=None, knot_time=None, knot_T=None):
    """Returns (points, rgba, kept candidate indices, stats) with stats = dict(candidates, invalid, out_of_range, overflowed,
    bad_time, track_overflowed, clamped); row_time = (scale, offset_s): the undistorting form."""
    pts, reason, u, v = unproject(img, cam)
    stats = {"candidates": len(u), "invalid": int((reason == 1).sum()), "out_of_range": int((reason == 2).sum()),
             "overflowed": int((reason == 3).sum()), "bad_time": 0, "track_overflowed": 0, "clamped": 0}
    kept = np.flatnonzero(reason == 0)
    pts = np.ascontiguousarray(pts[kept])
    if row_time is not None and len(kept):
        scale, offset_s = row_time
        with np.errstate(over="ignore", invalid="ignore"):
            t = np.float64(offset_s) + v[kept].astype(np.float64) * np.float64(scale)
        good = np.isfinite(t)
        stats["bad_time"] = int((~good).sum())
        pts, kept, t = pts[good], kept[good], t[good]
        pts, clamped = U.undistort_points(pts, t, knot_time, knot_T)
        fin = np.isfinite(pts).all(1)
        stats["track_overflowed"] = int((~fin).sum())
        stats["clamped"] = int((clamped & fin).sum())
        pts, kept = np.ascontiguousarray(pts[fin]), kept[fin]
    return pts, colours(img, u[kept], v[kept], constant_rgba), kept, stats


def dropped(stats):
    return stats["invalid"] + stats["out_of_range"] + stats["overflowed"] + stats["bad_time"] + stats["track_overflowed"]


# ---- builders -------------------------------------------------------------------------------------------------------
SPECIALS_16 = np.array([0, 1, 65535], np.uint16)
MIN_DEPTH, MAX_DEPTH = 0.25, 8.0                                    # (both exact in f32)
SPECIALS_32 = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-40, 3e38, MIN_DEPTH, MAX_DEPTH], F)


def rows(values, pad, fill):
    """the bytes of an image whose rows are the rows of `values` (a [h][w] or [h][w][c] array) and `pad` bytes of `fill`"""
    h = values.shape[0]
    body = np.ascontiguousarray(values).view(np.uint8).reshape(h, -1)
    out = np.full((h, body.shape[1] + pad), fill, np.uint8)
    out[:, :body.shape[1]] = body
    return out.reshape(-1), body.shape[1] + pad


def planted_depths(width, height, encoding, seed):
    """[h][w] depths (uint16 counts of a millimetre / f32 metres): ordinary ranges of 0.3 .. 7.9 m, about one pixel in five
    one of the encoding's special values, every one of them planted where the image has the room"""
    rng = np.random.default_rng(seed)
    n = width * height
    specials = SPECIALS_16 if encoding == DEPTH_16UC1 else SPECIALS_32
    metres = rng.uniform(0.3, 7.9, n)
    z = np.round(metres * 1000).astype(np.uint16) if encoding == DEPTH_16UC1 else metres.astype(F)
    pick = rng.random(n) < 0.2
    z[pick] = specials[rng.integers(0, len(specials), int(pick.sum()))]
    if n >= len(specials):
        z[rng.permutation(n)[:len(specials)]] = specials
    elif n:
        z[:] = specials[(seed + np.arange(n)) % len(specials)]
    return z.reshape(height, width)


def planted_image(width, height, encoding, seed, row_pad=0, color_kind=COLOR_NONE, color_pad=0):
    if width * height == 0:
        return Image(width, height, encoding, b"", None, color_kind, None if color_kind == COLOR_NONE else b"")
    z = planted_depths(width, height, encoding, seed)
    depth, row_step = rows(z, row_pad, 0xAB)
    color, color_row_step = None, 0
    if color_kind != COLOR_NONE:
        px = np.random.default_rng(seed + 1000).integers(0, 256, (height, width, COLOR_BPP[color_kind]), dtype=np.uint8)
        color, color_row_step = rows(px, color_pad, 0xCD)
    return Image(width, height, encoding, depth, row_step, color_kind, color, color_row_step)


def camera_for(width, height, **kw):
    """a pinhole model for an image of this size whose principal point is off the pixel grid"""
    f = 0.9 * max(width, height, 2)
    return Camera(f, f * 1.01, (width - 1) / 2 + 0.3, (height - 1) / 2 - 0.2, **kw)


T_ROOM_OPTICAL = np.array([0.5, -0.5, 0.5, -0.5, 0.1, -0.05, 0.02], F)   # optical z forward = the room's x, x right = -y, y down = -z


def room_frame(width, height, encoding, seed, color_kind=COLOR_RGB8, row_pad=2, color_pad=1):
    """a depth camera inside the room of tests/scan_msg_scenes.py looking along its x axis: (image, camera); regions without
    depth (a corner rectangle, a band of rows) and speckle are 0 / NaN as a driver leaves them"""
    from tests import scan_msg_scenes as S
    rng = np.random.default_rng(4000 + seed)
    cam = Camera(0.9 * width, 0.9 * width, width / 2 - 0.41, height / 2 - 0.37, min_depth_m=0.3, max_depth_m=6.0)
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    a, b = ((u - cam.cx) / cam.fx).reshape(-1), ((v - cam.cy) / cam.fy).reshape(-1)
    z = S._room_hits(np.stack([np.ones_like(a), -a, -b], 1))[:, 0].reshape(height, width) + rng.normal(0, 0.002, (height, width))
    hole = rng.random((height, width)) < 0.02
    hole[: height // 5, : width // 4] = True
    hole[height // 2 + 3: height // 2 + 9] = True
    if encoding == DEPTH_16UC1:
        z = np.round(z * 1000).astype(np.uint16)
        z[hole] = 0
    else:
        z = z.astype(F)
        z[hole] = np.nan
    depth, row_step = rows(z, row_pad, 0xAB)
    color, color_row_step = None, 0
    if color_kind != COLOR_NONE:
        color, color_row_step = rows(rng.integers(0, 256, (height, width, COLOR_BPP[color_kind]), dtype=np.uint8), color_pad, 0xCD)
    return Image(width, height, encoding, depth, row_step, color_kind, color, color_row_step), cam


def as_cloud(img, cam, points):
    """the candidates' points (NaN rows: holes) as an organised PointCloud2 of 16-byte pcl::PointXYZ, wc x hc"""
    from tests import scan_msg_scenes as S
    wc, hc = -(-img.width // cam.stride_u), -(-img.height // cam.stride_v)
    return S.Msg(wc, hc, 16, S.FIELDS["xyz16"]).fill(np.random.default_rng(7), points)
