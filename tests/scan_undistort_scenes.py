"""Messages with a per-point time field and pose tracks for the scan undistortion tests, generated from a seed: the
layouts of the issue (an aligned driver cloud, a 4- but not 8-aligned f64 time, unaligned f32 and f64 times, padded rows),
with the values the rules single out planted -- times equal to a knot, one f64 step either side of a knot, times before
and after the track, NaN and +-Inf times, NaN / Inf / -0.0 coordinates."""
import numpy as np

from tests import scan_msg_scenes as S
from tests import scan_undistort_ref as U

F = np.float32
STAMP = 1.7e9 + 0.25                                   # the message stamp of the layouts whose time is absolute

# name -> (point_step, fields, time kind, time offset, scale, offset_s)
LAYOUTS = {
    "driver48": (48, S.FIELDS["driver48"], U.TIME_UINT32, 20, 1e-9, 0.0),
    "step36_f64_at20": (36, S.XYZ + [("intensity", 12, S.FLOAT32, 1), ("timestamp", 20, S.FLOAT64, 1)], U.TIME_FLOAT64, 20, 1.0, -STAMP),
    "step27_f32_at17": (27, S.FIELDS["unaligned19_rgb"] + [("time", 17, S.FLOAT32, 1)], U.TIME_FLOAT32, 17, 1.0, 0.0),
    "step27_f64_at19": (27, S.FIELDS["unaligned19_intensity"] + [("timestamp", 19, S.FLOAT64, 1)], U.TIME_FLOAT64, 19, 1.0, -STAMP),
}
T_LO, T_HI = 0.01, 0.09                                # the track's span inside a sweep of [0, 0.1] s


def put_time(m, f, raw):
    """raw: uint32 / float32 / float64 per point, as the field's kind"""
    if f.kind == U.TIME_FLOAT64:
        w = np.ascontiguousarray(raw, np.float64).view(np.uint64)
        m.put(f.offset, (w & np.uint64(0xffffffff)).astype(np.uint32))
        m.put(f.offset + 4, (w >> np.uint64(32)).astype(np.uint32))
    else:
        m.put(f.offset, np.ascontiguousarray(raw, np.uint32 if f.kind == U.TIME_UINT32 else F))


def raw_times(f, seconds):
    """the raw field values that stand for `seconds` after the sweep's start"""
    if f.kind == U.TIME_UINT32:
        return np.round(np.asarray(seconds) / f.scale).astype(np.uint32)
    if f.kind == U.TIME_FLOAT32:
        return np.asarray(seconds, F)
    return np.asarray(seconds, np.float64) - f.offset_s


def message(name, width, height, seed=0, row_pad=0, specials=True):
    """-> (msg, time field, xyz as planted [n][3] f32): random points and times over [0, 0.1] s; with `specials`
    plant_specials' coordinates and, in a float time field, NaN and +-Inf times on points that survive the first filter"""
    step, fields, kind, off, scale, offset_s = LAYOUTS[name]
    rng = np.random.default_rng(7000 + seed)
    m = S.Msg(width, height, step, fields, row_pad)
    f = U.TimeField(kind, off, scale, offset_s)
    xyz = rng.uniform(-8, 8, (m.n, 3)).astype(F)
    if specials and m.n >= 64:
        S.plant_specials(xyz)
    colour = rng.uniform(-100, 12000, m.n).astype(F) if m.color_kind == S.COLOR_INTENSITY else \
        rng.integers(0, 2 ** 32, m.n, dtype=np.uint64).astype(np.uint32)
    m.fill(rng, xyz, colour)
    sec = rng.uniform(0.0, 0.1, m.n)
    sec[: min(m.n, 16)] = np.linspace(0.03, 0.07, min(m.n, 16))          # (small messages: times inside the track)
    raw = raw_times(f, sec)
    if specials and m.n >= 64 and kind != U.TIME_UINT32:
        ok = np.flatnonzero(np.isfinite(xyz).all(1))
        raw[ok[20]], raw[ok[21]], raw[ok[22]] = np.nan, np.inf, -np.inf
        raw[5] = np.nan                                                  # (and on a point the first filter may have dropped)
    put_time(m, f, raw)
    return m, f, xyz


def knots(m, f, K, seed=0):
    """-> (knot_time [K] f64, knot_T [K][7] f32): K knots over [T_LO, T_HI], up to 12 of them planted on the times of
    points of the message: equal to one, one f64 step above one, one f64 step below one, in turn"""
    rng = np.random.default_rng(8000 + seed)
    t = U.times(m, m.base(), f)
    inside = np.unique(t[np.isfinite(t) & (t > T_LO) & (t < T_HI)])
    pick = rng.choice(inside, min(K, 12, len(inside)), replace=False)
    pick[1::3] = np.nextafter(pick[1::3], np.inf)
    pick[2::3] = np.nextafter(pick[2::3], -np.inf)
    kt = np.unique(np.concatenate([np.linspace(T_LO, T_HI, K - len(pick)), pick]))
    while len(kt) < K:                                                   # (a planted time met a regular one)
        kt = np.unique(np.concatenate([kt, rng.uniform(T_LO, T_HI, K - len(kt))]))
    # a smooth motion, 2 m/s and 1 rad/s about a tilted axis, with jitter; quaternions only roughly of unit length
    ang = 1.0 * (kt - kt[0]) + rng.normal(0, 1e-3, K)
    axis = np.array([0.1, -0.2, 0.97])
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], 1)
    pos = np.stack([2.0 * (kt - kt[0]), 0.3 * np.sin(20 * kt), 0.05 * np.cos(9 * kt)], 1) + rng.normal(0, 1e-3, (K, 3))
    return kt, np.concatenate([q, pos], 1).astype(F)


def overflow_scene():
    """xyz16-like driver48 message whose points of 3e38 overflow under a 90-degree knot and survive under the identity
    knot before it: -> (msg, time field, knot_time, knot_T, expected overflowed, expected clamped)"""
    m, f, xyz = message("driver48", 300, 1, seed=99, specials=False)
    rng = np.random.default_rng(99)
    big = np.arange(10, 300, 7)
    xyz[big] = F(3e38) * np.sign(rng.uniform(-1, 1, (len(big), 3))).astype(F)
    xyz[big, 2] = 0.0
    for k, o in enumerate((m.offset_x, m.offset_y, m.offset_z)):
        m.put(o, xyz[:, k])
    sec = np.full(m.n, 0.05)
    sec[::2] = 0.005                                                     # before the track: the identity knot alone
    sec[1::4] = 0.095                                                    # after it: the 90-degree knot alone
    put_time(m, f, raw_times(f, sec))
    kt = np.array([0.02, 0.08])
    s = np.sqrt(0.5)
    kT = np.array([[1, 0, 0, 0, 0, 0, 0], [s, 0, 0, s, 0.1, 0.2, 0.3]], F)
    return m, f, kt, kT
