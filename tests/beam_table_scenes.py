"""The scenes of the beam-table tests: the room of tests/range_image_scenes.py seen by four table sensors -- 64 x 8 clockwise
with column 0 backwards, a non-uniform ascending table (gaps 0.02 to 0.2 rad) and offsets of mixed sign up to 0.07 rad;
128 x 16 counter-clockwise, descending, with a FINITE limit smaller than some half gaps (holes between rows); 64 x 1 with a
finite limit; 4 x 2 -- with the planted points of the uniform scenes and one in a hole between two rows.  SENSOR_MODELS and
SENSOR_CASES: tables of real sizes -- 128 rows with a cluster 1.2 mrad apart, 256 rows, a dense centre, clusters with holes
between them, a row of 2e-5 rad, two rows 1e-3 rad apart (profiles/range_image_sensor_sizes.txt).  Needs no device."""
import numpy as np

from tests import beam_table_ref as B
from tests import range_image_scenes as S
from tests.range_image_scenes import IDENTITY, TILTED, config, far_from_origin, message, pose, quat, ranges, sensor_poses, track  # noqa: F401

F = np.float32

_E8 = -0.35 + np.concatenate([[0.0], np.cumsum([0.2, 0.12, 0.05, 0.02, 0.03, 0.08, 0.2])])
_O8 = [0.07, -0.03, 0.0, 0.05, -0.07, 0.02, -0.01, 0.04]
_G16 = [0.04, 0.1, 0.05, 0.08, 0.04, 0.05, 0.09, 0.04, 0.07, 0.05, 0.1, 0.04, 0.06, 0.05, 0.08]
_E16 = 0.5 - np.concatenate([[0.0], np.cumsum(_G16)])
_O16 = 0.02 * np.sin(np.arange(16) * 1.3)

MODELS = {
    "64x8": B.BeamModel(64, _E8, _O8, S.PI32, 1),
    "128x16": B.BeamModel(128, _E16, _O16, -1.0, 0, row_half_extent_max_rad=0.03),
    "64x1": B.BeamModel(64, [0.05], [0.03], 0.4, 0, row_half_extent_max_rad=0.15),
    "4x2": B.BeamModel(4, [-0.3, 0.3], [0.05, -0.05], 0.5, 1),
}
# the same height as "64x8", another table: a rebuild into one handle must not meet the table held
OTHER_64x8 = B.BeamModel(64, _E8[::-1] * 0.9, _O8[::-1], S.PI32, 1)


def _rows(first, gaps):
    return first + np.concatenate([[0.0], np.cumsum(gaps)])


# 128 rows: 12 mrad apart at the edges, a cluster of 48 gaps of 1.2 mrad in the middle (a third of a coarse bin each)
_E128 = _rows(-0.5, [0.012] * 40 + [0.0012] * 48 + [0.012] * 39)
# 256 rows, 3.1 mrad apart with a seeded jitter of at most 0.8 mrad, given descending
_E256 = (np.linspace(-0.4, 0.4, 256) + np.random.default_rng(256).uniform(-0.0008, 0.0008, 256))[::-1]
# 32 rows: a centre of 19 gaps of 5.8 mrad, edges of up to 60 mrad
_E32 = _rows(-0.23, [0.06, 0.045, 0.03, 0.02, 0.012, 0.008] + [0.0058] * 19 + [0.008, 0.012, 0.02, 0.03, 0.045, 0.06])
# 64 rows in 16 clusters of four: 3 mrad apart within a cluster, 25 mrad between clusters
_E64 = _rows(-0.26, ([0.003] * 3 + [0.025]) * 15 + [0.003] * 3)
assert len(_E128) == 128 and len(_E32) == 32 and len(_E64) == 64 and (np.diff(_E256.astype(F)) < 0).all()

# the sizes of real sensors, up to the 256 rows vgx_range_image_check_beams accepts
SENSOR_MODELS = {
    "1024x128_clustered": B.BeamModel(1024, _E128, 0.02 * np.sin(1.3 * np.arange(128)), -1.0, 0),
    "512x256_descending": B.BeamModel(512, _E256, 0.01 * np.cos(0.7 * np.arange(256)), 0.4, 1),
    "2048x32_dense_centre": B.BeamModel(2048, _E32, 0.03 * np.cos(2.1 * np.arange(32)), S.PI32, 1),
    # a limit of 4 mrad: the rows of a cluster meet (half a gap is 1.5 mrad), holes of 17 mrad lie between the clusters
    "900x64_holes": B.BeamModel(900, _E64, 0.015 * np.sin(0.9 * np.arange(64)), 2.0, 0, row_half_extent_max_rad=0.004),
    # a row of 2e-5 rad: 256 bins over it would be 1.28e7 bins per radian, the coarse table's scale is clamped to 1e6
    "256x1_thin": B.BeamModel(256, [0.05], [0.03], 0.4, 0, row_half_extent_max_rad=1e-5),
    "64x2_close": B.BeamModel(64, [0.1, 0.101], [0.01, -0.01], -2.0, 1),
}
# the uniform 2048 x 128 sensor of the uniform scenes as a table: its image is the uniform model's
UNIFORM_2048x128 = B.uniform_as_table(S.SENSOR_MODELS["2048x128"])


def hole(model):
    """an elevation in the middle of the widest hole between two rows (None: the rows meet)"""
    gap = model.lo[1:].astype(np.float64) - model.hi[:-1].astype(np.float64)
    if not len(gap) or gap.max() <= 0:
        return None
    k = int(gap.argmax())
    return 0.5 * (float(model.lo[k + 1]) + float(model.hi[k]))


def scan(model, T=IDENTITY, seed=3, planted=True, jitter=0.3):
    """-> (points [n][3] f32 in the sensor frame, rgba [n] u32): one return per pixel, up to `jitter` column pitches and
    `jitter` of the row's half extent off its centre, in a shuffled order, then the planted points"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(model.height), np.arange(model.width), indexing="ij")
    lo, hi = model.extent(v)
    e = model.row_elevation_rad.astype(np.float64)[v]
    d_el = rng.uniform(-jitter, jitter, u.shape) * np.minimum(e - lo, hi - e)
    dirs = model.direction(u + rng.uniform(-jitter, jitter, u.shape), v, d_el).reshape(-1, 3)
    pts = (dirs * ranges(dirs, T)[:, None]).astype(F)
    keep = np.ones(len(pts), bool)
    if planted:
        keep[rng.choice(len(pts), len(pts) // 16, replace=False)] = False      # pixels without a return
    pts = pts[keep][rng.permutation(int(keep.sum()))]
    extra = []
    if planted:
        extra.append(np.zeros(3))                                               # a zero-length point
        c = model.direction(5 % model.width, min(3, model.height - 1))
        extra += [c * 0.7, c * 0.9, c * 0.7]                                    # one pixel: nearer, farther, bit-equal
        extra.append(model.direction(9 % model.width, min(2, model.height - 1)) * 0.05)   # shorter than min_ray_length_m
        extra.append(np.array([0.02, 0.01, 1.0]))                               # above every row
        extra += [np.array([-1.0, 1e-7, 0.05]), np.array([-1.0, -1e-7, 0.05]), np.array([-1.2, 0.0, -0.1])]   # the seam
        extra.append(pts[7].astype(np.float64))                                 # a scan point twice: equal ranges
        h = hole(model)
        if h is not None:
            extra.append(np.array([np.cos(h) * 0.6, np.cos(h) * 0.8, np.sin(h)]) * 1.3)   # in a hole between two rows
    pts = np.concatenate([pts, np.array(extra, F).reshape(-1, 3)])
    rgba = rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)
    return pts, rgba


# the nine configurations of the uniform test, the uniform sensors replaced by the table sensors of the same size
CASES = S.CASES


# name -> (sensor table, the room far from the origin, vps): two scans into one layer each, 0.1 m voxels, rays up to 4 m
SENSOR_CASES = {
    "1024x128_clustered": ("1024x128_clustered", False, 8),
    "512x256_descending": ("512x256_descending", False, 8),
    "2048x32_dense_centre": ("2048x32_dense_centre", False, 8),
    "900x64_holes": ("900x64_holes", False, 8),
    "256x1_thin": ("256x1_thin", False, 8),
    "64x2_close": ("64x2_close", False, 8),
    "1024x128_clustered_vps16": ("1024x128_clustered", False, 16),
    "900x64_holes_far": ("900x64_holes", True, 8),
}
# the fields of view of these two (2e-5 and 2e-3 rad) hold too few voxel centres within 4 m for a thousand updates
THIN = ("256x1_thin", "64x2_close")


def sensor_scan(m, k):
    """scan k (0 or 1) of a sensor case -> (points, rgba)"""
    return S.sensor_scan(m, k, scan)


def sensor_case(name):
    """-> (BeamModel, [(points, rgba, pose)] of the two scans, Config, voxel size, vps)"""
    return S.sensor_case(name, SENSOR_CASES, SENSOR_MODELS, scan)


def case(name):
    """-> (BeamModel, points, rgba, Config, pose, voxel size, vps)"""
    model, T, vs, vps, over = CASES[name]
    room_pose = TILTED if name == "far_tilted" else T
    pts, rgba = scan(MODELS[model], room_pose)
    return MODELS[model], pts, rgba, config(vs, **over), np.asarray(T, F), vs, vps
