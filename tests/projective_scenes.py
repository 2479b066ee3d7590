"""The scenes of the projective-integration tests: a 48 x 32 depth camera in a room corner whose back wall has an opening
onto a far wall beyond max_ray_length_m, with holes planted in the frame.  Rendered in f64 from plane equations; needs no
device.  World axes are the optical frame's at the identity pose: x right, y down, z forward."""
import numpy as np

from tests import projective_ref as P

F = np.float32
WIDTH, HEIGHT = 48, 32
CAMERA = dict(fx=38.0, fy=37.0, cx=23.3, cy=15.6)
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], F)
# left wall, right wall, ceiling, floor, back wall (with the opening), far wall: (axis, offset)
PLANES = [(0, -1.5), (0, 2.0), (1, -1.2), (1, 1.0), (2, 2.6), (2, 6.5)]
OPENING = ((0.3, 1.2), (-0.9, 0.0))       # x and y range of the back wall's opening


def rotate(q, p):
    """q (w, x, y, z) applied to points p [..., 3], f64"""
    w, v = q[0], np.asarray(q[1:], np.float64)
    uv = 2.0 * np.cross(v, p)
    return p + w * uv + np.cross(v, uv)


def quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def qmul(a, b):
    aw, av, bw, bv = a[0], a[1:], b[0], b[1:]
    return np.concatenate([[aw * bw - av @ bv], aw * bv + bw * av + np.cross(av, bv)])


def pose(q, t):
    return np.concatenate([q, t]).astype(F)


TILTED = pose(qmul(quat([0, 1, 0], 0.5), quat([1, 0.2, 0], -0.3)), [0.2, -0.1, 0.15])
# the same room seen from a camera far from the origin: the world is moved with it (far_pose o TILTED)
FAR_Q, FAR_T = qmul(quat([0.3, 1, 0.2], 2.1), quat([0, 0, 1], 0.4)), np.array([-123.4, 57.8, -310.2])


def z_depth(T=IDENTITY, camera=CAMERA, width=WIDTH, height=HEIGHT):
    """[height][width] f64 z-depth of the room from pose T (world = the room's frame)"""
    T = np.asarray(T, np.float64)
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    dirs = np.stack([(u - camera["cx"]) / camera["fx"], (v - camera["cy"]) / camera["fy"], np.ones(u.shape)], -1)
    dw, o = rotate(T[:4], dirs), T[4:]
    best = np.full(u.shape, np.inf)
    for k, (axis, off) in enumerate(PLANES):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (off - o[axis]) / dw[..., axis]
        hit = o + t[..., None] * dw
        ok = (t > 1e-9) & (t < best)
        if k == 4:       # the back wall: not where the opening is
            ok &= ~((hit[..., 0] > OPENING[0][0]) & (hit[..., 0] < OPENING[0][1]) & (hit[..., 1] > OPENING[1][0]) & (hit[..., 1] < OPENING[1][1]))
        best = np.where(ok, t, best)
    return best


def colour_bytes(kind, width=WIDTH, height=HEIGHT, row_pad=0, seed=5):
    bpp = P.COLOR_BPP[kind]
    if bpp == 0:
        return None, 0
    rng = np.random.default_rng(seed)
    step = width * bpp + row_pad
    return rng.integers(0, 256, height * step, dtype=np.uint8), step


def frame(encoding, T=IDENTITY, color_kind=P.COLOR_NONE, row_pad=0, holes=True, width=WIDTH, height=HEIGHT, camera=CAMERA):
    """-> (Image, Camera): the room from T with holes planted (zeros for 16UC1; NaN, 0, -1 and +inf for 32FC1)"""
    z = z_depth(T, camera, width, height)
    bpp = P.DEPTH_BPP[encoding]
    step = width * bpp + row_pad
    buf = np.full((height, step), 0xA5, np.uint8)                        # (the padding is never read as a depth)
    if encoding == P.DEPTH_16UC1:
        px = np.round(z / 0.001).clip(0, 65535).astype("<u2")
        if holes:
            px[3:6, 4:9] = 0
            px[20, ::5] = 0
    else:
        px = z.astype("<f4")
        if holes:
            px[3:6, 4:9] = np.nan
            px[20, ::5] = 0.0
            px[11, 30:34] = -1.0
            px[25, 10:13] = np.inf
    buf[:, :width * bpp] = px.view(np.uint8).reshape(height, width * bpp)
    color, cstep = colour_bytes(color_kind, width, height, row_pad=(3 if row_pad else 0))
    img = P.Image(width, height, encoding, buf, step, color_kind, color, cstep if color is not None else None)
    return img, P.Camera(**camera)


def config(voxel_size, **kw):
    """truncation three voxels, rays up to 4 m (the far wall is a clearing return), the rest voxblox's defaults"""
    base = dict(default_truncation_distance=3 * voxel_size, max_ray_length_m=4.0, min_ray_length_m=0.1)
    base.update(kw)
    return P.Config(**base)


def far_from_origin(T):
    """the pose of a camera that sees the room as T does when the room itself sits at (FAR_Q, FAR_T)"""
    T = np.asarray(T, np.float64)
    return pose(qmul(FAR_Q, T[:4]), rotate(FAR_Q, T[4:]) + FAR_T)


# name -> (encoding, colour kind, row_pad, pose, voxel size, vps, config overrides): the single-frame cases of the GPU test
CASES = {
    "16uc1": (P.DEPTH_16UC1, P.COLOR_NONE, 0, IDENTITY, 0.1, 8, {}),
    "32fc1": (P.DEPTH_32FC1, P.COLOR_NONE, 0, IDENTITY, 0.1, 8, {}),
    "padded_rgb8": (P.DEPTH_16UC1, P.COLOR_RGB8, 6, TILTED, 0.1, 8, {}),
    "padded_odd_bgr8": (P.DEPTH_32FC1, P.COLOR_BGR8, 3, TILTED, 0.1, 8, {}),
    "rgba8_vps16": (P.DEPTH_16UC1, P.COLOR_RGBA8, 0, TILTED, 0.05, 16, {}),
    "bgra8_vps16_coarse": (P.DEPTH_32FC1, P.COLOR_BGRA8, 0, IDENTITY, 0.1, 16, {}),
    "mono8_fine": (P.DEPTH_32FC1, P.COLOR_MONO8, 0, TILTED, 0.05, 8, {}),
    "no_carving": (P.DEPTH_32FC1, P.COLOR_RGB8, 0, TILTED, 0.1, 8, dict(voxel_carving_enabled=0)),
    "no_clearing": (P.DEPTH_16UC1, P.COLOR_RGB8, 0, IDENTITY, 0.1, 8, dict(allow_clear=0)),
    "const_weight": (P.DEPTH_32FC1, P.COLOR_RGB8, 0, TILTED, 0.1, 8, dict(use_const_weight=1)),
    "no_dropoff": (P.DEPTH_16UC1, P.COLOR_RGB8, 0, TILTED, 0.1, 8, dict(use_weight_dropoff=0)),
    "far_tilted": (P.DEPTH_32FC1, P.COLOR_RGB8, 0, far_from_origin(TILTED), 0.1, 8, {}),
    "depth_gate": (P.DEPTH_32FC1, P.COLOR_NONE, 0, IDENTITY, 0.1, 8, dict(_camera=dict(min_depth_m=0.8, max_depth_m=3.0))),
}


def case(name):
    """-> (Image, Camera, Config, pose, voxel size, vps)"""
    encoding, kind, pad, T, vs, vps, over = CASES[name]
    over = dict(over)
    cam_over = over.pop("_camera", {})
    room_pose = TILTED if name == "far_tilted" else T
    img, cam = frame(encoding, room_pose, kind, pad)
    for k, v in cam_over.items():
        setattr(cam, k, v)
    return img, cam, config(vs, **over), np.asarray(T, F), vs, vps
