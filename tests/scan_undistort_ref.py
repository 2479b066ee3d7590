"""numpy restatement of the undistorting scan decode (include/voxgraph_amd.h, "Scan undistortion").  Written from the rules
in the header, not from the kernel: the time field assembled byte by byte, t = offset_s + raw * scale in f64, the segment
by np.searchsorted(side="right") - 1, the two knots' transforms of the point in f32 one rounding per operation, the
linear blend, and the three filters in their order.  numpy never contracts a multiply and an add."""
import numpy as np

from tests import scan_msg_ref as R

F = np.float32
TIME_UINT32, TIME_FLOAT32, TIME_FLOAT64 = 0, 1, 2


class TimeField:
    def __init__(self, kind, offset, scale=1.0, offset_s=0.0):
        self.kind, self.offset, self.scale, self.offset_s = kind, offset, float(scale), float(offset_s)

    def capi(self, capi):
        return capi.scan_time_field(self.kind, self.offset, self.scale, self.offset_s)


def transform_point(T, p):
    """kindr::minimal's transform as vgx_tsdf_internal.h states it (Eigen's quaternion-vector product, then the
    translation), f32, in its association.  T [n][7] or [7], p [n][3]."""
    T = np.asarray(T, F).reshape(-1, 7)
    qw, qx, qy, qz, tx, ty, tz = (T[:, k] for k in range(7))
    px, py, pz = (np.asarray(p, F)[:, k] for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        uvx, uvy, uvz = qy * pz - qz * py, qz * px - qx * pz, qx * py - qy * px
        uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
        ccx, ccy, ccz = qy * uvz - qz * uvy, qz * uvx - qx * uvz, qx * uvy - qy * uvx
        return np.stack([(px + qw * uvx + ccx) + tx, (py + qw * uvy + ccy) + ty, (pz + qw * uvz + ccz) + tz], 1).astype(F)


def times(msg, base, f):
    """t of the points at byte addresses `base`: f64"""
    data = np.frombuffer(msg.data, np.uint8)
    lo = R.field_u32(data, base, f.offset)
    if f.kind == TIME_UINT32:
        raw = lo.astype(np.float64)
    elif f.kind == TIME_FLOAT32:
        raw = lo.view(F).astype(np.float64)
    elif f.kind == TIME_FLOAT64:
        hi = R.field_u32(data, base, f.offset + 4)
        raw = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)).view(np.float64)
    else:
        raise ValueError("unknown time kind")
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float64(f.offset_s) + raw * np.float64(f.scale)


def segment(t, knot_time):
    """-> (k, a f32, clamped) for finite times t"""
    kt = np.asarray(knot_time, np.float64)
    K = len(kt)
    cnt = np.searchsorted(kt, t, side="right")
    k = np.maximum(cnt - 1, 0)
    inside = (cnt > 0) & (cnt < K)
    a = np.zeros(len(t), F)
    ki = k[inside]
    a[inside] = ((t[inside] - kt[ki]) / (kt[ki + 1] - kt[ki])).astype(F)
    clamped = (cnt == 0) | ((cnt == K) & (t > kt[K - 1]))
    return k, a, clamped


def undistort_points(p, t, knot_time, knot_T):
    """the point rule on finite points p [n][3] f32 with finite times t -> (out [n][3] f32, clamped)"""
    knot_T = np.asarray(knot_T, F).reshape(-1, 7)
    k, a, clamped = segment(t, knot_time)
    out = transform_point(knot_T[k], p)
    b = np.flatnonzero(a != F(0))
    if len(b):
        with np.errstate(over="ignore", invalid="ignore"):
            g0, g1 = out[b], transform_point(knot_T[k[b] + 1], p[b])
            out[b] = g0 + a[b, None] * (g1 - g0)
    return out, clamped


def decode(msg, f, knot_time, knot_T, **cfg):
    """Returns (points, rgba, kept message indices, stats) with stats = dict(not_finite, bad_time, overflowed, clamped)."""
    pts, rgba, kept = R.decode(msg, **cfg)
    n = msg.width * msg.height
    stats = {"not_finite": n - len(kept), "bad_time": 0, "overflowed": 0, "clamped": 0}
    if len(kept) == 0:
        return pts, rgba, kept, stats
    base = (kept // msg.width) * np.int64(msg.row_step) + (kept % msg.width) * np.int64(msg.point_step)
    t = times(msg, base, f)
    good = np.isfinite(t)
    stats["bad_time"] = int((~good).sum())
    pts, rgba, kept, t = pts[good], rgba[good], kept[good], t[good]
    out, clamped = undistort_points(pts, t, knot_time, knot_T)
    fin = np.isfinite(out).all(1)
    stats["overflowed"] = int((~fin).sum())
    stats["clamped"] = int((clamped & fin).sum())
    return np.ascontiguousarray(out[fin]), np.ascontiguousarray(rgba[fin]), kept[fin], stats
