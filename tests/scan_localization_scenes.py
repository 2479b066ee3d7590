"""The scenes the scan-localisation tests share (tests/scan_localization_ref.py): random posed submaps that overlap one
another -- block sets with holes, ~10 % invalid voxels, general-quaternion poses, voxel sizes that differ -- with sensor-frame
points of every kind, and the ASYMMETRIC room: scan_registration_ref's box room plus a full-height pillar, built by the CPU
oracle's integrator from six scans, its ESDF by tests/esdf_ref.py, and a seventh scan taken elsewhere to be localised.  (The
plain room maps onto itself under a half turn about its centre: a global search cannot tell the two poses apart.)"""
import math

import numpy as np

from oracle import synth
from tests import scan_registration_ref as SR
from tests.projected_map_ref import F, inverse, quat_rotate

VOXEL_SIZES = (0.1, 0.12, 0.08)


def random_pose(rng, spread=0.3):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.array([*q, *rng.uniform(-spread, spread, 3)], F)


def compose(Ta, Tb):
    """Ta o Tb of two 7-vector poses, in f64, rounded to f32 once"""
    a, b = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    w1, x1, y1, z1 = a[:4]
    w2, x2, y2, z2 = b[:4]
    q = [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]
    u = np.array([x1, y1, z1])
    t = b[4:] + 2.0 * np.cross(u, np.cross(u, b[4:]) + w1 * b[4:]) + a[4:]
    return np.array([*q, *t], np.float64).astype(F)


def random_submaps(rng, vps, n_submaps=3):
    """-> (submaps [n] SubmapData, T_M_S [n][7] f32): <= 30 blocks each out of a 4 x 4 x 2 box with holes, shuffled slots,
    ~10 % zero weights / unobserved voxels, centred near the mission origin so that they overlap"""
    submaps, poses = [], []
    for k in range(n_submaps):
        pool = synth.dense_block_index((-2, -2, -1), (4, 4, 2))
        bi = pool[rng.random(len(pool)) < 0.8]
        bi = bi[rng.permutation(len(bi))]
        n, nv = len(bi), vps ** 3
        assert 0 < n <= 30
        td = rng.uniform(-0.3, 0.3, (n, nv)).astype(F)
        tw = np.where(rng.random((n, nv)) < 0.1, F(0), rng.uniform(0.1, 10, (n, nv)).astype(F)).astype(F)
        ed = rng.uniform(-0.5, 0.5, (n, nv)).astype(F)
        eo = (rng.random((n, nv)) < 0.9).astype(np.uint8)
        submaps.append(synth.SubmapData(VOXEL_SIZES[k % 3] * (16 // vps), vps, bi.astype(np.int32), td, tw, ed, eo, np.zeros(4)))
        poses.append(random_pose(rng))
    return submaps, np.array(poses, F)


def _submap_points(rng, d, n):
    """submap-frame points: inside the blocks, outside the map, on block faces and on voxel centres / faces"""
    vs, bs = F(d.voxel_size), F(d.voxel_size * d.vps)
    lo, hi = d.block_index.min(0) * bs, (d.block_index.max(0) + 1) * bs
    inside = rng.uniform(lo, hi, (n, 3))
    outside = rng.uniform(lo - 2 * bs, hi + 2 * bs, (n // 4, 3))
    faces = rng.uniform(lo, hi, (n // 4, 3))
    ax = rng.integers(0, 3, len(faces))
    faces[np.arange(len(faces)), ax] = np.round(faces[np.arange(len(faces)), ax] / bs) * bs
    grid = np.floor(rng.uniform(lo, hi, (n // 4, 3)) / vs) * vs + rng.choice([0.0, 0.5], (n // 4, 3)) * vs
    return np.concatenate([inside, outside, faces, grid]).astype(F)


def sensor_points(rng, submaps, poses, n, T_M_C):
    """[>= n][3] f32 sensor-frame points of pose T_M_C: every submap's kinds of points, shuffled, with NaN / inf / 3e38
    strewn in"""
    per = -(-n // len(submaps))
    pm = np.concatenate([(quat_rotate(T[:4], _submap_points(rng, d, per)) + T[4:]).astype(F) for d, T in zip(submaps, poses)])
    pm = pm[rng.permutation(len(pm))]
    qi, ti = inverse(T_M_C)
    pc = (quat_rotate(qi, pm) + ti).astype(F)
    bad = rng.random(len(pc)) < 0.02
    pc[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf, 3e38], int(bad.sum())).astype(F)
    return np.ascontiguousarray(pc, F)


# ---------------------------------------------------------------------------
# the asymmetric room
# ---------------------------------------------------------------------------
PILLAR_LO, PILLAR_HI = np.array([2.0, 1.5]), np.array([3.0, 2.5])       # x, y: full height
TRUE_POSE = np.array([-1.3, -0.9, 0.02, 0.7])                           # where the scan to localise was taken
MAX_ABS_DISTANCE = 1.9                                                  # below the ESDF's 2 m plateau
GRID_X, GRID_Y, GRID_YAWS, GRID_Z = np.arange(-3.5, 4.01, 0.5), np.arange(-2.5, 3.01, 0.5), 24, 0.02
EXPECTED_CELL = (-1.0, -1.0, 2.0 * math.pi * 3 / 24)                    # the hypothesis next to TRUE_POSE (yaw 0.785)


def room_scan(p4, n_az=256, n_el=16):
    """scan_registration_ref.room_scan's beams in the room with the pillar: the rays' first hit"""
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, n_az, endpoint=False) + (2 * np.pi / n_az) / 3.0,
                         np.linspace(-0.3, 0.3, n_el) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    c, s = math.cos(p4[3]), math.sin(p4[3])
    dw = np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1], d[:, 2]], -1)
    o = np.asarray(p4[:3], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dw > 0, (SR.ROOM_HI - o) / dw, np.where(dw < 0, (SR.ROOM_LO - o) / dw, np.inf)).min(1)
        t1, t2 = (PILLAR_LO - o[:2]) / dw[:, :2], (PILLAR_HI - o[:2]) / dw[:, :2]
        near, far = np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)
    hit = (near <= far) & (near > 0)
    return (d * np.where(hit, np.minimum(t, near), t)[:, None]).astype(F)


_ROOM = []


def room_submap():
    """SubmapData of the asymmetric room: the TSDF layer the CPU oracle's FastTsdfIntegrator builds from scans 0..5 at
    scan_registration_ref.scan_pose(k), and its ESDF by esdf_ref; computed once and shared (nobody writes to it)"""
    if not _ROOM:
        from oracle import pyoracle as orc
        from tests import esdf_ref
        layer = orc.TsdfLayer(SR.VOXEL_SIZE, SR.VPS)
        integrator = orc.FastTsdfIntegrator(orc.voxgraph_tsdf_config(), layer)
        for k in range(6):
            integrator.integratePointCloud(SR.pose7(SR.scan_pose(k)), room_scan(SR.scan_pose(k)))
        bi, d, w, _ = layer.download()
        ed, eo = esdf_ref.esdf_from_tsdf(SR.VOXEL_SIZE, SR.VPS, bi, d, w)
        for a in (bi, d, w, ed, eo):
            a.setflags(write=False)
        _ROOM.append(synth.SubmapData(SR.VOXEL_SIZE, SR.VPS, bi, d, w, ed, eo, np.zeros(4)))
    return _ROOM[0]


def room_scans():
    """the six scans that build the room: [(T_S_C [7] f32, points [n][3] f32)]"""
    return [(SR.pose7(SR.scan_pose(k)), room_scan(SR.scan_pose(k))) for k in range(6)]


def scan_to_localize():
    return room_scan(TRUE_POSE)
