"""The scenes of the range-image tests: a spinning LiDAR of 64 x 8 or 128 x 16 pixels in a room of 3.5 x 2.8 x 1.8 m whose
+x wall has an opening onto a far wall beyond max_ray_length_m, with planted points: pixels without a return, a
zero-length point, second returns in a pixel (nearer, farther and bit-equal), a point above the rows, a return shorter
than min_ray_length_m, points on the +-pi seam.  Rendered in f64 from plane equations; needs no device.  The sensor
frame is x forward, y left, z up.  SENSOR_MODELS and SENSOR_CASES: the same room seen by sensors of real sizes, up to the
4096 x 256 the check accepts (profiles/range_image_sensor_sizes.txt)."""
import numpy as np

from tests import range_image_ref as R
from tests.projective_scenes import far_from_origin, pose, qmul, quat, rotate  # noqa: F401 (re-exported)

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], F)
# (axis, offset): -x, +x (with the opening), -y, +y, floor, ceiling, the far wall
PLANES = [(0, -1.5), (0, 2.0), (1, -1.2), (1, 1.6), (2, -0.8), (2, 1.0), (0, 6.5)]
OPENING = ((-0.5, 0.7), (-0.4, 0.5))       # y and z range of the +x wall's opening
PI32 = float(R.PI)

MODELS = {
    # Ouster-like: clockwise, column 0 looks backwards, the top row first
    "64x8": R.Model(64, 8, PI32, 1, 0.35, -0.35),
    # counter-clockwise from an odd azimuth, the bottom row first
    "128x16": R.Model(128, 16, -1.0, 0, -0.4, 0.5),
}
TILTED = pose(qmul(quat([0, 0, 1], 0.6), quat([1, 0.3, 0], 0.12)), [0.2, -0.1, 0.15])
# the sizes of real sensors, up to the limit vgx_range_image_check accepts (pitches down to 1.5 mrad)
SENSOR_MODELS = {
    # clockwise, column 0 looks backwards, the top row first, +-22.5 degrees
    "1024x64": R.Model(1024, 64, PI32, 1, 0.3927, -0.3927),
    # counter-clockwise from an odd azimuth, the bottom row first
    "2048x128": R.Model(2048, 128, -1.0, 0, -0.4, 0.5),
    # the limit: pitches of 1.53 mrad in both angles
    "4096x256": R.Model(4096, 256, 2.5, 1, 0.196, -0.195),
    # a width that is no power of two, +-15 degrees
    "1800x16": R.Model(1800, 16, 0.7, 0, -0.2618, 0.2618),
    # a field of view of 0.02 rad: the two cones nearly meet
    "512x4": R.Model(512, 4, 0.0, 1, -0.01, 0.01),
    # looking up only: both cones on one side, the top one near the axis
    "360x32_up": R.Model(360, 32, 0.3, 0, 0.6, 1.5),
}


def ranges(dirs, T=IDENTITY):
    """f64 range of the room along sensor-frame unit directions dirs [..., 3] from pose T (layer frame = the room's)"""
    T = np.asarray(T, np.float64)
    dw, o = rotate(T[:4], np.asarray(dirs, np.float64)), T[4:]
    best = np.full(dw.shape[:-1], np.inf)
    for k, (axis, off) in enumerate(PLANES):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (off - o[axis]) / dw[..., axis]
        hit = o + t[..., None] * dw
        ok = (t > 1e-9) & (t < best)
        if k == 1:       # the +x wall: not where the opening is
            ok &= ~((hit[..., 1] > OPENING[0][0]) & (hit[..., 1] < OPENING[0][1]) & (hit[..., 2] > OPENING[1][0]) & (hit[..., 2] < OPENING[1][1]))
        best = np.where(ok, t, best)
    return best


def scan(model, T=IDENTITY, seed=3, planted=True, jitter=0.3):
    """-> (points [n][3] f32 in the sensor frame, rgba [n] u32): one return per pixel, up to `jitter` pitches off its
    centre, in a shuffled order, then the planted points"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(model.height), np.arange(model.width), indexing="ij")
    uj = u + rng.uniform(-jitter, jitter, u.shape)
    vj = v + rng.uniform(-jitter, jitter, v.shape)
    dirs = model.centre(uj, vj).reshape(-1, 3)
    pts = (dirs * ranges(dirs, T)[:, None]).astype(F)
    keep = np.ones(len(pts), bool)
    if planted:
        keep[rng.choice(len(pts), len(pts) // 16, replace=False)] = False      # pixels without a return
    pts = pts[keep][rng.permutation(int(keep.sum()))]
    extra = []
    if planted:
        extra.append(np.zeros(3))                                               # a zero-length point
        c = model.centre(5, 3)
        extra += [c * 0.7, c * 0.9, c * 0.7]                                    # one pixel: nearer, farther, bit-equal
        extra.append(model.centre(9, 2) * 0.05)                                 # shorter than min_ray_length_m
        extra.append(np.array([0.02, 0.01, 1.0]))                               # above every row
        extra += [np.array([-1.0, 1e-7, 0.05]), np.array([-1.0, -1e-7, 0.05]), np.array([-1.2, 0.0, -0.1])]   # the seam
        extra.append(pts[7].astype(np.float64))                                 # a scan point twice: equal ranges
    pts = np.concatenate([pts, np.array(extra, F).reshape(-1, 3)])
    rgba = rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)
    return pts, rgba


def message(points, rgba):
    """a PointXYZRGB PointCloud2's bytes (point_step 16: x y z f32, then PCL's packed colour) and its layout keywords"""
    pts, rgba = np.ascontiguousarray(points, F).reshape(-1, 3), np.ascontiguousarray(rgba, np.uint32).reshape(-1)
    buf = np.zeros((len(pts), 16), np.uint8)
    buf[:, :12] = pts.view(np.uint8).reshape(-1, 12)
    c = rgba[:, None].view(np.uint8).reshape(-1, 4)                              # r g b a
    buf[:, 12], buf[:, 13], buf[:, 14], buf[:, 15] = c[:, 2], c[:, 1], c[:, 0], c[:, 3]
    layout = dict(width=len(pts), height=1, point_step=16, row_step=16 * len(pts), offset_x=0, offset_y=4, offset_z=8,
                  color_kind=1, color_offset=12)
    return buf.reshape(-1), layout


def config(voxel_size, **kw):
    """truncation three voxels, rays up to 4 m (the far wall is a clearing return), the rest voxblox's defaults"""
    base = dict(default_truncation_distance=3 * voxel_size, max_ray_length_m=4.0, min_ray_length_m=0.1)
    base.update(kw)
    return R.Config(**base)


# name -> (model, pose, voxel size, vps, config overrides): the single-scan cases of the GPU test
CASES = {
    "ouster": ("64x8", IDENTITY, 0.1, 8, {}),
    "ouster_tilted": ("64x8", TILTED, 0.1, 8, {}),
    "ccw_vps16": ("128x16", TILTED, 0.1, 16, {}),
    "ccw_yaw180": ("128x16", pose(quat([0, 0, 1], np.pi), [0.3, 0.2, -0.1]), 0.1, 8, {}),
    "no_carving": ("64x8", TILTED, 0.1, 8, dict(voxel_carving_enabled=0)),
    "no_clearing": ("64x8", IDENTITY, 0.1, 16, dict(allow_clear=0)),
    "const_weight": ("128x16", IDENTITY, 0.1, 8, dict(use_const_weight=1)),
    "no_dropoff": ("64x8", TILTED, 0.1, 8, dict(use_weight_dropoff=0)),
    "far_tilted": ("64x8", far_from_origin(TILTED), 0.1, 8, {}),
}


def case(name):
    """-> (Model, points, rgba, Config, pose, voxel size, vps)"""
    model, T, vs, vps, over = CASES[name]
    room_pose = TILTED if name == "far_tilted" else T
    pts, rgba = scan(MODELS[model], room_pose)
    return MODELS[model], pts, rgba, config(vs, **over), np.asarray(T, F), vs, vps


def track(n=5):
    """poses along a short track through the room"""
    return [pose(quat([0, 0, 1], 0.15 * k), [0.1 * k, -0.05 * k, 0.02 * k]) for k in range(n)]


# name -> (sensor model, the room far from the origin, vps): two scans into one layer each, 0.1 m voxels, rays up to 4 m
SENSOR_CASES = {
    "1024x64": ("1024x64", False, 8),
    "2048x128": ("2048x128", False, 8),
    "4096x256": ("4096x256", False, 8),
    "1800x16": ("1800x16", False, 8),
    "512x4": ("512x4", False, 8),
    "360x32_up": ("360x32_up", False, 8),
    "1024x64_vps16": ("1024x64", False, 16),
    "4096x256_far": ("4096x256", True, 8),
}


def sensor_poses(far=False):
    """-> [(the pose the room is seen from, the pose the scan is integrated at)]: TILTED, then a moved pose of track()"""
    return [(np.asarray(T, F), np.asarray(far_from_origin(T) if far else T, F)) for T in (TILTED, track()[2])]


def sensor_scan(m, k, scan_fn=None):
    """scan k (0 or 1) of a sensor case -> (points, rgba); the same near the origin and far from it"""
    return (scan_fn or scan)(m, sensor_poses()[k][0], seed=3 + k)


def sensor_case(name, cases=None, models=None, scan_fn=None):
    """-> (Model, [(points, rgba, pose)] of the two scans, Config, voxel size, vps); the three keywords: the beam tables'"""
    model, far, vps = (cases or SENSOR_CASES)[name]
    m = (models or SENSOR_MODELS)[model]
    scans = [(*sensor_scan(m, k, scan_fn), T) for k, (_, T) in enumerate(sensor_poses(far))]
    return m, scans, config(0.1), 0.1, vps
