"""The synthetic scenes of tests/test_layer_cloud_gpu.py, kept apart so that tests/test_layer_cloud_cpu.py can check on the
CPU that none of them passes on nothing.  A scene is one block set with an ESDF (distance, observed), a TSDF (distance,
weight) and colours over it, and the cloud configurations it is viewed with; every source kind views the same arrays."""
import numpy as np

from oracle import synth
from tests import layer_cloud_ref as R

F = np.float32
SURFACE = F(0.6)


class Scene:
    def __init__(self, voxel_size, vps, bi, d, o, w, rgba, configs):
        self.voxel_size, self.vps, self.bi, self.d, self.o, self.w, self.rgba = voxel_size, vps, bi, d, o, w, rgba
        self.configs = configs


def reference(sc, cfg, source):
    """the restatement for one source kind: "esdf", "tsdf" (a finished submap's layers) or "layer" (a vgx_tsdf_layer)"""
    esdf = source == "esdf"
    return R.layer_cloud(sc.voxel_size, sc.vps, sc.bi, sc.d, sc.o if esdf else sc.w, esdf=esdf, rgba=sc.rgba, **cfg)


def sources_of(cfg):
    return ("layer",) if cfg.get("kind", R.DISTANCE) == R.SURFACE_COLOR else ("esdf", "tsdf", "layer")


def census(sc, cfg):
    """the least over the source kinds of (points, voxels, contributing blocks, blocks the slice rejects)"""
    out = None
    for source in sources_of(cfg):
        _, _, _, per = reference(sc, cfg, source)
        rejected = 0
        if cfg.get("slice_axis", -1) >= 0:
            c = R.voxel_centres(sc.voxel_size, sc.vps, sc.bi)[:, :, cfg["slice_axis"]]
            reach = F(0.5) * F(sc.voxel_size) + R.SLICE_TOLERANCE
            rejected = int((~(np.abs(c - F(cfg["slice_value"])) <= reach).any(1)).sum())
        row = (int(per.sum()), int(sc.d.size), int((per > 0).sum()), rejected)
        out = row if out is None else tuple(min(a, b) for a, b in zip(out, row))
    return out


def _fill(rng, n, vps):
    nv = vps ** 3
    d = rng.uniform(-1.0, 2.0, (n, nv)).astype(F)
    o = (rng.random((n, nv)) < 0.85).astype(np.uint8)
    o[rng.random((n, nv)) < 0.02] = 200                                    # observed is "!= 0", not "== 1"
    w = np.where(rng.random((n, nv)) < 0.15, F(0), rng.uniform(0.0, 5.0, (n, nv)).astype(F)).astype(F)
    # planted boundaries: weights at and just above the threshold, |d| at and just below the band, non-finite distances
    w[rng.random((n, nv)) < 0.02] = R.MIN_WEIGHT
    w[rng.random((n, nv)) < 0.02] = np.nextafter(R.MIN_WEIGHT, F(1))
    w[rng.random((n, nv)) < 0.005] = F(np.nan)
    for value in (SURFACE, -SURFACE, np.nextafter(SURFACE, F(0)), -np.nextafter(SURFACE, F(0)), F(np.nan), F(np.inf), F(-np.inf),
                  F(0.0), F(-0.0)):
        d[rng.random((n, nv)) < 0.01] = value
    rgba = rng.integers(0, 256, (n, nv, 4), dtype=np.uint8)
    return d, o, w, rgba


def _blocks(rng, box_min, box_dims, n):
    pool = synth.dense_block_index(box_min, box_dims)
    return np.ascontiguousarray(pool[rng.permutation(len(pool))[:n]], dtype=np.int32)    # shuffled, with holes


def _views(planes):
    """the three kinds without a slice; then every slice as a distance view and with a surface band"""
    cfgs = [dict(kind=R.DISTANCE), dict(kind=R.SURFACE_DISTANCE, surface_distance=SURFACE),
            dict(kind=R.SURFACE_COLOR, surface_distance=SURFACE)]
    for axis, value in planes:
        cfgs.append(dict(kind=R.DISTANCE, slice_axis=axis, slice_value=float(value)))
        cfgs.append(dict(kind=R.SURFACE_DISTANCE, surface_distance=SURFACE, slice_axis=axis, slice_value=float(value)))
        cfgs.append(dict(kind=R.SURFACE_COLOR, surface_distance=SURFACE, slice_axis=axis, slice_value=float(value)))
    return cfgs


def _random_scene(seed, vps, box_min, n=60, voxel_size=0.1):
    rng = np.random.default_rng(seed)
    bi = _blocks(rng, box_min, (6, 6, 4), n)
    d, o, w, rgba = _fill(rng, n, vps)
    c = R.voxel_centres(voxel_size, vps, bi)
    planes = []
    for axis in range(3):
        mid = int(np.median(bi[:, axis]))
        b = int(np.flatnonzero(bi[:, axis] == mid)[0])
        planes.append((axis, c[b, (3 + axis) * (1, vps, vps * vps)[axis], axis]))   # a row centre of a middle block
    return Scene(voxel_size, vps, bi, d, o, w, rgba, _views(planes))


def _boundary_scene(vps):
    """voxel_size 0.125: centres, block faces and half voxels are exact in f32, so the slice's edge cases can be planted"""
    rng = np.random.default_rng(100 + vps)
    vs = 0.125
    bi = _blocks(rng, (-2, -2, -2), (4, 4, 4), 40)
    d, o, w, rgba = _fill(rng, len(bi), vps)
    bs = vps * vs
    reach = F(0.5) * F(vs) + R.SLICE_TOLERANCE
    planes = []
    for axis in range(3):
        face = float(bs * 1)                                     # the face between blocks 0 and 1
        planes += [(axis, face),                                 # half a voxel from the rows on either side: both
                   (axis, F(face) + F(5e-7)),                    # inside the tolerance: both
                   (axis, F(face) + F(2e-6)),                    # beyond it: the upper row alone
                   (axis, -bs + 3 * vs),                         # a voxel boundary inside block -1: rows 2 and 3
                   (axis, F(0.5 * vs) - reach),                  # block 0's row 0 exactly at the reach: kept
                   (axis, F(0.5 * vs) - reach - F(2.0 ** -27))]     # one ulp of the reach further: dropped
    return Scene(vs, vps, bi, d, o, w, rgba, _views(planes))


SCENES = {
    "random_vps8": lambda: _random_scene(8, 8, (-3, -3, -2)),
    "random_vps16": lambda: _random_scene(16, 16, (-3, -3, -2), n=40),
    "far_vps8": lambda: _random_scene(48, 8, (40, -46, 43)),
    "far_vps16": lambda: _random_scene(56, 16, (-46, 40, -44), n=40),
    "boundary_vps8": lambda: _boundary_scene(8),
    "boundary_vps16": lambda: _boundary_scene(16),
}
