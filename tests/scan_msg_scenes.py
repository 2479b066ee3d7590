"""sensor_msgs/PointCloud2 messages for the scan tests: the layouts a driver or PCL produces (and some only the
specification allows), with the values the decode rules single out planted in them.  Everything is generated from a
seed; bytes no field of the layout covers (other fields, point and row padding) are random, so a decode that reads the
wrong place does not go unnoticed."""
import numpy as np

from tests.scan_msg_ref import COLOR_INTENSITY, COLOR_NONE, COLOR_RGB

F = np.float32
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = range(1, 9)     # sensor_msgs/PointField datatypes


class Msg:
    """A PointCloud2: the header, the named fields (name, offset, datatype, count) and the bytes."""

    def __init__(self, width, height, point_step, fields, row_pad=0):
        self.width, self.height, self.point_step = width, height, point_step
        self.row_step = width * point_step + row_pad
        self.fields = list(fields)
        self.is_bigendian = 0
        off = {name: o for name, o, _, _ in self.fields}
        self.offset_x, self.offset_y, self.offset_z = off["x"], off["y"], off["z"]
        # pointcloud_integrator.cpp:35-63: a field named rgb wins, else intensity, else none
        self.color_kind = COLOR_RGB if "rgb" in off else (COLOR_INTENSITY if "intensity" in off else COLOR_NONE)
        self.color_offset = off.get("rgb", off.get("intensity", 0))
        self.data = np.zeros(height * self.row_step, np.uint8)

    @property
    def n(self):
        return self.width * self.height

    def base(self):
        i = np.arange(self.n, dtype=np.int64)
        return (i // self.width) * self.row_step + (i % self.width) * self.point_step

    def put(self, offset, words):
        """the 4-byte little-endian field at `offset` of every point"""
        w = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
        at = self.base() + offset
        for k in range(4):
            self.data[at + k] = ((w >> np.uint32(8 * k)) & np.uint32(0xff)).astype(np.uint8)

    def fill(self, rng, xyz, colour=None):
        self.data[:] = rng.integers(0, 256, len(self.data), dtype=np.uint8)
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        for k, o in enumerate((self.offset_x, self.offset_y, self.offset_z)):
            self.put(o, xyz[:, k])
        if colour is not None and self.color_kind != COLOR_NONE:
            self.put(self.color_offset, colour)
        return self

    def layout(self, capi):
        return capi.scan_layout(width=self.width, height=self.height, point_step=self.point_step, row_step=self.row_step,
                                offset_x=self.offset_x, offset_y=self.offset_y, offset_z=self.offset_z,
                                color_kind=self.color_kind, color_offset=self.color_offset, is_bigendian=self.is_bigendian)


XYZ = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1)]
FIELDS = {
    "xyz16": XYZ,                                                               # pcl::PointXYZ
    "xyzi32": XYZ + [("intensity", 16, FLOAT32, 1)],                            # pcl::PointXYZI
    "xyzrgb32": XYZ + [("rgb", 16, FLOAT32, 1)],                                # pcl::PointXYZRGB
    "driver48": XYZ + [("intensity", 16, FLOAT32, 1), ("t", 20, UINT32, 1), ("reflectivity", 24, UINT16, 1),
                       ("ring", 26, UINT16, 1), ("ambient", 28, UINT16, 1), ("range", 32, UINT32, 1)],
    "unaligned19_rgb": [("x", 1, FLOAT32, 1), ("y", 5, FLOAT32, 1), ("z", 9, FLOAT32, 1), ("rgb", 13, FLOAT32, 1)],
    "unaligned19_intensity": [("x", 1, FLOAT32, 1), ("y", 5, FLOAT32, 1), ("z", 9, FLOAT32, 1), ("intensity", 13, FLOAT32, 1)],
}
STEP = {"xyz16": 16, "xyzi32": 32, "xyzrgb32": 32, "driver48": 48, "unaligned19_rgb": 19, "unaligned19_intensity": 19}

# intensities the grey scale singles out, for the default range [0, 10000]: NaN (-> min), +-Inf, negative, -0.0, 0, 5000
# (h = 0.5, h * 255 = 127.5 exactly: the one half the f32 grid reaches), values just either side of it, max, beyond max,
# and levels whose fraction is above one half (a truncating cast loses them)
SPECIAL_INTENSITIES = np.array([np.nan, np.inf, -np.inf, -5.0, -0.0, 0.0, 5000.0, np.nextafter(F(5000), F(0)),
                                np.nextafter(F(5000), F(1e9)), 10000.0, 20000.0, 1e30, 39.0, 9990.0, 2530.0, 19.7, 58.9], F)


def plant_specials(xyz):
    """NaN, +Inf and -Inf separately in each coordinate, all three at once, and -0.0 (finite: kept, bit for bit), at
    fixed places spread over the cloud.  Returns the indices that must be dropped."""
    n = len(xyz)
    dropped = []
    at = iter(range(3, n, max(1, n // 23)))
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            i = next(at)
            xyz[i, axis] = bad
            dropped.append(i)
    i = next(at)
    xyz[i] = np.nan
    dropped.append(i)
    for axis in range(3):
        xyz[next(at), axis] = -0.0
    xyz[0, 2] = np.nan                                      # the first and the last point of the message
    xyz[n - 1, 0] = -np.inf
    return sorted(set(dropped + [0, n - 1]))


def small(name, seed=0, width=37, height=5, row_pad=0):
    """a cloud of random points in the named layout with every special value planted"""
    rng = np.random.default_rng(seed)
    m = Msg(width, height, STEP[name], FIELDS[name], row_pad)
    xyz = rng.uniform(-8, 8, (m.n, 3)).astype(F)
    plant_specials(xyz)
    colour = None
    if m.color_kind == COLOR_RGB:
        colour = rng.integers(0, 2 ** 32, m.n, dtype=np.uint64).astype(np.uint32)
    elif m.color_kind == COLOR_INTENSITY:
        colour = rng.uniform(-100, 12000, m.n).astype(F)
        kept = np.flatnonzero(np.isfinite(xyz).all(1))
        colour[kept[1:1 + len(SPECIAL_INTENSITIES)]] = SPECIAL_INTENSITIES          # on points that survive the filter
    return m.fill(rng, xyz, colour)


def _room_hits(dirs):
    """where rays from the origin along dirs leave the box [-4, 4.5] x [-3, 3.5] x [-1, 2]"""
    lo, hi = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dirs > 0, hi / dirs, np.where(dirs < 0, lo / dirs, np.inf)).min(1)
    return dirs * t[:, None]


def lidar(seed=0, rows=64, cols=1024, name="xyzi32", row_pad=0):
    """a rows x cols spinning LiDAR inside a room (row = beam, column = azimuth), XYZI; about 3 % of the beams have no
    return (NaN), some return +Inf, some lie beyond the maximum range"""
    rng = np.random.default_rng(1000 + seed)
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, cols, endpoint=False) + (2 * np.pi / cols) / 3.0 + 0.01 * seed,
                         np.linspace(-0.3, 0.3, rows) + 0.004)
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    xyz = (_room_hits(dirs) + rng.normal(0, 0.004, dirs.shape)).astype(F)
    xyz[rng.random(len(xyz)) < 0.03] = np.nan
    xyz[rng.random(len(xyz)) < 0.002, 1] = np.inf
    xyz[::97] *= F(4.0)
    m = Msg(cols, rows, STEP[name], FIELDS[name], row_pad)
    inten = rng.uniform(0, 12000, m.n).astype(F)
    inten[rng.random(m.n) < 0.01] = np.nan
    return m.fill(rng, xyz, inten if m.color_kind == COLOR_INTENSITY else rng.integers(0, 2 ** 32, m.n, dtype=np.uint64).astype(np.uint32))


def depth(seed=0, rows=480, cols=640, name="xyzrgb32", row_pad=0):
    """an organised rows x cols depth image of the same room (pinhole, looking along +x), XYZRGB: whole regions without
    depth (a corner rectangle, a band of rows, a disc) and speckle are NaN, as a depth camera's driver leaves them"""
    rng = np.random.default_rng(2000 + seed)
    v, u = np.meshgrid((np.arange(rows) - rows / 2 + 0.37) / (0.9 * cols), (np.arange(cols) - cols / 2 + 0.41) / (0.9 * cols),
                       indexing="ij")
    dirs = np.stack([np.ones_like(u), -u, -v], -1).reshape(-1, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    xyz = (_room_hits(dirs) + rng.normal(0, 0.002, dirs.shape)).astype(F).reshape(rows, cols, 3)
    xyz[: rows // 5, : cols // 4] = np.nan
    xyz[rows // 2 + 7: rows // 2 + 31] = np.nan
    rr, cc = np.ogrid[:rows, :cols]
    xyz[(rr - 0.7 * rows) ** 2 + (cc - 0.8 * cols) ** 2 < (0.12 * rows) ** 2] = np.nan
    xyz[rng.random((rows, cols)) < 0.02] = np.nan
    m = Msg(cols, rows, STEP[name], FIELDS[name], row_pad)
    return m.fill(rng, xyz.reshape(-1, 3), rng.integers(0, 2 ** 32, m.n, dtype=np.uint64).astype(np.uint32))


def lattice(seed=0, name="xyzrgb32"):
    """points on a coarse lattice 1.3 m apart in front of the sensor, a third of them not finite: without carving the
    truncation bands (0.25 m) of two rays never share a voxel, so the racing integrator's result has one legal value"""
    rng = np.random.default_rng(3000 + seed)
    g = np.arange(-4, 5) * 1.3
    xyz = np.array([(x + 0.03, y - 0.02, 6.0 + 0.1 * np.sin(x * y)) for x in g for y in g], F)
    xyz[rng.permutation(len(xyz))[: len(xyz) // 3], rng.integers(0, 3)] = np.nan
    m = Msg(len(xyz), 1, STEP[name], FIELDS[name])
    return m.fill(rng, xyz, rng.integers(0, 2 ** 32, m.n, dtype=np.uint64).astype(np.uint32))


def aged_pair(seed=0, width=1031, height=67):
    """two XYZI messages of one size for the handle-age tests (tests/test_handle_age_gpu.py): 69 077 points in 68 tiles of
    1024 -- a ragged last tile, and tiles 65 to 67 look back through a second window of 64 tiles -- each with about 30 %
    of its points not finite, chosen from different seeds: every tile keeps another number of points in the two, so no
    tile's sum in one message is its sum in the other"""
    pair = []
    for k in range(2):
        rng = np.random.default_rng(4000 + 2 * seed + k)
        m = Msg(width, height, STEP["xyzi32"], FIELDS["xyzi32"])
        xyz = rng.uniform(-8, 8, (m.n, 3)).astype(F)
        bad = np.flatnonzero(rng.random(m.n) < 0.3)
        xyz[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
        pair.append(m.fill(rng, xyz, rng.uniform(-100, 12000, m.n).astype(F)))
    return pair


# every layout the decode tests walk: name -> builder
LAYOUTS = {
    "xyz16": lambda: small("xyz16", 1),
    "xyzi32": lambda: small("xyzi32", 2),
    "xyzrgb32": lambda: small("xyzrgb32", 3),
    "driver48": lambda: small("driver48", 4, width=128, height=16),
    "unaligned19_rgb": lambda: small("unaligned19_rgb", 5),
    "unaligned19_intensity": lambda: small("unaligned19_intensity", 6, width=1031, height=3, row_pad=7),
    "padded_rows_aligned": lambda: small("xyzi32", 7, width=50, height=9, row_pad=24),
    "padded_rows_unaligned": lambda: small("xyzrgb32", 8, width=50, height=9, row_pad=5),
    "one_row_of_one": lambda: Msg(1, 1, 16, XYZ).fill(np.random.default_rng(9), [[1.0, -0.0, 3.0]]),
    "depth_480x640": lambda: depth(0),
    "depth_padded": lambda: depth(1, row_pad=64),
    "lidar_64x1024": lambda: lidar(0),
    "lidar_driver48": lambda: lidar(1, name="driver48"),
}
