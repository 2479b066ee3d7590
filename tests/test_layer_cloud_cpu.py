"""Layer point clouds without a GPU: the numpy restatement (tests/layer_cloud_ref.py) against points written out by hand,
the scenes of the GPU tests checked not to pass on nothing, and the new symbols exported by libvoxgraph_amd.so and
declared in include/voxgraph_amd.h."""
import os
import re

import numpy as np
import pytest

from tests import layer_cloud_ref as R
from tests import layer_cloud_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SYMBOLS = ["vgx_cloud_config_default", "vgx_cloud_create", "vgx_cloud_destroy", "vgx_cloud_stats", "vgx_cloud_download",
           "vgx_cloud_device_pointers", "vgx_submap_layer_cloud", "vgx_tsdf_layer_cloud", "vgx_evaluate_layers_rmse_cloud"]


def _two_blocks():
    """vps 8, voxel_size 0.125 (a block is 1 m): blocks (0,0,0) and (0,0,1), nothing observed but what a test plants"""
    bi = np.array([[0, 0, 0], [0, 0, 1]], np.int32)
    d = np.zeros((2, 512), F)
    o = np.zeros((2, 512), np.uint8)
    return bi, d, o


def _lin(x, y, z):
    return x + 8 * (y + 8 * z)


def test_surface_band_by_hand():
    bi, d, o = _two_blocks()
    # five observed voxels in block 0, one in block 1; the band is |d| < 0.25
    plant = [(0, _lin(1, 0, 0), 0.1), (0, _lin(0, 1, 0), 0.25), (0, _lin(2, 2, 2), -0.2), (0, _lin(7, 7, 7), -0.25),
             (0, _lin(3, 0, 0), np.nan), (1, _lin(0, 0, 0), 0.249)]
    for b, v, val in plant:
        d[b, v], o[b, v] = val, 1
    d[0, _lin(5, 5, 5)] = 0.01                                             # in the band but not observed
    xyz, inten, col, per = R.layer_cloud(0.125, 8, bi, d, o, R.SURFACE_DISTANCE, surface_distance=0.25)
    # linear-index order inside block 0: (1,0,0) = 1 before (2,2,2) = 146; then block 1
    assert xyz.tolist() == [[0.1875, 0.0625, 0.0625], [0.3125, 0.3125, 0.3125], [0.0625, 0.0625, 1.0625]]
    assert inten.tolist() == [F(0.1), F(-0.2), F(0.249)] and col is None and per.tolist() == [2, 1]
    # every observed voxel, NaN included, in the distance view
    xyz, inten, _, per = R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE)
    assert per.tolist() == [5, 1] and np.isnan(inten[1]) and xyz[1].tolist() == [0.4375, 0.0625, 0.0625]    # (3,0,0) = 3


def test_slice_through_a_known_row_by_hand():
    bi, d, o = _two_blocks()
    o[:] = 1
    d[:] = np.arange(1024, dtype=F).reshape(2, 512)
    # z = 0.3125 is the centre of row z = 2 of block 0: that row's 64 voxels, nothing of block 1
    xyz, inten, _, per = R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=2, slice_value=0.3125)
    assert per.tolist() == [64, 0] and np.all(xyz[:, 2] == F(0.3125))
    assert inten.tolist() == list(range(128, 192))
    assert xyz[:9, 0].tolist() == [0.0625 + 0.125 * i for i in range(8)] + [0.0625] and xyz[8, 1] == F(0.1875)
    # on the x axis: the column x = 7 of both blocks, 64 voxels each, in linear order
    xyz, inten, _, per = R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=0, slice_value=0.95)
    assert per.tolist() == [64, 64] and np.all(xyz[:, 0] == F(0.9375)) and inten[:3].tolist() == [7, 15, 23]


def test_slice_on_a_block_face_by_hand():
    bi, d, o = _two_blocks()
    o[:] = 1
    # z = 1 is the face between the blocks: the centres 0.9375 and 1.0625 are exactly half a voxel away, both rows pass
    _, _, _, per = R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=2, slice_value=1.0)
    assert per.tolist() == [64, 64]
    # just above the face, within the 1e-6 tolerance: still both; beyond it: the upper row alone
    assert R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=2, slice_value=1.0 + 5e-7)[3].tolist() == [64, 64]
    assert R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=2, slice_value=1.0 + 2e-6)[3].tolist() == [0, 64]
    # exactly at the reach (not strictly): plane = centre - (vs / 2 + 1e-6) in f32
    reach = F(0.0625) + F(1e-6)
    plane = F(0.0625) - reach
    assert F(0.0625) - plane == reach
    assert R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=2, slice_value=plane)[3].tolist() == [64, 0]
    assert R.layer_cloud(0.125, 8, bi, d, o, R.DISTANCE, slice_axis=2, slice_value=plane - F(2.0 ** -27))[3].tolist() == [0, 0]   # one ulp of the reach further


def test_tsdf_weight_threshold_and_colours_by_hand():
    bi, d, _ = _two_blocks()
    w = np.zeros((2, 512), F)
    rgba = np.arange(2 * 512 * 4, dtype=np.uint32).astype(np.uint8).reshape(2, 512, 4)
    w[0, 3] = F(1e-3)                                   # at the threshold: not observed
    w[0, 4] = np.nextafter(F(1e-3), F(1))
    w[1, 9] = F(2.0)
    w[1, 10] = F(np.nan)
    xyz, inten, col, per = R.layer_cloud(0.125, 8, bi, d, w, R.SURFACE_COLOR, esdf=False, rgba=rgba)
    assert per.tolist() == [1, 1] and xyz.tolist() == [[0.5625, 0.0625, 0.0625], [0.1875, 0.1875, 1.0625]]
    assert col.tolist() == [rgba[0, 4].tolist(), rgba[1, 9].tolist()]


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_gpu_scenes_do_not_pass_on_nothing(name):
    """what tests/test_layer_cloud_gpu.py asserts of every scene, met by the restatement alone"""
    sc = S.SCENES[name]()
    for cfg in sc.configs:
        n, n_vox, contributing, rejected = S.census(sc, cfg)
        assert 0 < n < n_vox, (name, cfg, n)
        if cfg.get("slice_axis", -1) >= 0:
            assert contributing >= 2 and rejected >= 1, (name, cfg, contributing, rejected)


def test_new_symbols_are_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from voxgraph_amd import capi
    lib = capi.load()
    text = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    declared = set(re.findall(r"VGX_API\s+[\w\s\*]+?\b(vgx_\w+)\s*\(", text))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    cfg = capi.cloud_config()
    assert (cfg.kind, cfg.slice_axis, cfg.slice_value) == (0, -1, 0.0)
    assert F(cfg.surface_distance) == F(0.6) and F(cfg.min_weight) == R.MIN_WEIGHT
    for macro, value in (("VGX_CLOUD_DISTANCE", 0), ("VGX_CLOUD_SURFACE_DISTANCE", 1), ("VGX_CLOUD_SURFACE_COLOR", 2)):
        assert re.search(rf"#define {macro} {value}\b", text)
    assert (capi.CLOUD_DISTANCE, capi.CLOUD_SURFACE_DISTANCE, capi.CLOUD_SURFACE_COLOR) == (R.DISTANCE, R.SURFACE_DISTANCE, R.SURFACE_COLOR)
