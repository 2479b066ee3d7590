"""The scenes of the beam-table tests: the room of tests/range_image_scenes.py seen by four table sensors -- 64 x 8 clockwise
with column 0 backwards, a non-uniform ascending table (gaps 0.02 to 0.2 rad) and offsets of mixed sign up to 0.07 rad;
128 x 16 counter-clockwise, descending, with a FINITE limit smaller than some half gaps (holes between rows); 64 x 1 with a
finite limit; 4 x 2 -- with the planted points of the uniform scenes and one in a hole between two rows.  Needs no device."""
import numpy as np

from tests import beam_table_ref as B
from tests import range_image_scenes as S
from tests.range_image_scenes import IDENTITY, TILTED, config, far_from_origin, message, pose, quat, ranges, track  # noqa: F401

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


def case(name):
    """-> (BeamModel, points, rgba, Config, pose, voxel size, vps)"""
    model, T, vs, vps, over = CASES[name]
    room_pose = TILTED if name == "far_tilted" else T
    pts, rgba = scan(MODELS[model], room_pose)
    return MODELS[model], pts, rgba, config(vs, **over), np.asarray(T, F), vs, vps
