"""The planar map's numpy restatement (tests/planar_map_ref.py) against grids written out by hand, its distance passes
against a brute-force integer transform over all cell pairs, the scenes of the GPU tests checked not to pass on nothing,
and the new symbols exported by libvoxgraph_amd.so and declared in include/voxgraph_amd.h."""
import os
import re

import numpy as np
import pytest

from tests import planar_map_ref as R
from tests import planar_map_scenes as S

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vgx_planar_map_config_default", "vgx_planar_map_create", "vgx_planar_map_destroy", "vgx_tsdf_layer_planar_map",
           "vgx_submap_layer_planar_map", "vgx_planar_map_stats", "vgx_planar_map_set_timing", "vgx_planar_map_pass_ms", "vgx_planar_map_download", "vgx_planar_map_device_pointers"]


def _two_blocks():
    """vps 2, voxel_size 0.5 (block 1.0): blocks (0, 0, 0) and (1, 0, 0), every voxel written out.  Linear index x fastest:
    [z0y0x0, z0y0x1, z0y1x0, z0y1x1, z1y0x0, z1y0x1, z1y1x0, z1y1x1]; row centres z = 0.25 and 0.75."""
    bi = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    d = np.array([[0.5, -0.5, 0.5, np.nan, 0.25, 0.5, -0.0, 0.5],
                  [0.5, 0.5, 0.5, 0.5, 0.75, 0.5, 0.0, 0.5]], F)
    o = np.array([[1, 1, 1, 1, 1, 1, 1, 0],
                  [1, 0, 1, 1, 1, 0, 1, 1]], np.uint8)
    return bi, d, o


def test_the_restatement_on_a_grid_written_out_by_hand():
    bi, d, o = _two_blocks()
    m = R.planar_map(0.5, 2, bi, d, o, True, z_min=0.0, z_max=1.0, max_distance_m=1.0)
    assert (m.x0, m.y0, m.W, m.H, m.R) == (0, 0, 4, 2, 2)
    # cell (x, y): its voxels upwards ->  (0,0): 0.5, 0.25 free  (1,0): -0.5 occ, 0.5  (2,0): 0.5, 0.75  (3,0): unobserved x2
    #                                    (0,1): 0.5, -0.0 occ   (1,1): NaN, unobserved (2,1): 0.5, 0.0 occ (3,1): 0.5, 0.5
    assert m.state.tolist() == [[1, 2, 1, 0], [2, 0, 2, 1]]
    assert m.occupancy.tolist() == [[0, 100, 0, -1], [100, -1, 100, 0]]
    assert R.same(m.clearance, np.array([[0.25, -0.5, 0.5, 0.0], [-0.0, 0.0, 0.0, 0.5]], F))
    assert R.same(m.height, np.array([[0.0, 0.25, 0.0, 0.0], [0.75, 0.0, 0.75, 0.0]], F))
    assert m.n_occ.tolist() == [[0, 1, 0, 0], [1, 0, 1, 0]] and m.n_free.tolist() == [[2, 1, 2, 0], [1, 0, 1, 2]]
    assert m.counts == (2, 3, 3)
    r2 = F(np.sqrt(F(2))) * F(0.5)
    assert R.same(m.distance, np.array([[0.5, 0.0, 0.5, r2], [0.0, 0.5, 0.0, 0.5]], F))
    # unknown cells as obstacles; the lower row alone (z_max on its centre: included; just below it: nothing)
    m = R.planar_map(0.5, 2, bi, d, o, True, z_min=0.0, z_max=1.0, max_distance_m=1.0, unknown_is_obstacle=1)
    assert R.same(m.distance, np.array([[0.5, 0.0, 0.5, 0.0], [0.0, 0.0, 0.0, 0.5]], F))
    m = R.planar_map(0.5, 2, bi, d, o, True, z_min=0.25, z_max=0.25)
    assert m.state.tolist() == [[1, 2, 1, 0], [1, 0, 1, 1]] and R.same(m.height, np.array([[0, 0.25, 0, 0], [0, 0, 0, 0]], F))
    m = R.planar_map(0.5, 2, bi, d, o, True, z_min=0.0, z_max=np.nextafter(F(0.25), F(0)))
    assert (m.W, m.H, m.counts) == (0, 0, (0, 0, 0))
    # min_free_voxels = 2; a box that is not block-aligned and reaches outside the layer; the clip at one cell
    m = R.planar_map(0.5, 2, bi, d, o, True, z_min=0.0, z_max=1.0, min_free_voxels=2, use_box=1, cell_min=(-1, 1), cell_dim=(4, 2),
                     max_distance_m=0.4)
    assert m.state.tolist() == [[0, 2, 0, 2], [0, 0, 0, 0]] and m.R == 1
    assert R.same(m.distance, np.array([[0.4, 0.0, 0.4, 0.0], [0.4, 0.4, 0.4, 0.4]], F))
    # the TSDF's observed rule: weight > min_weight, strictly; a NaN weight is not observed
    w = np.where(o != 0, F(1.0), F(0.0)).astype(F)
    w[0, 1], w[0, 6], w[1, 6] = R.MIN_WEIGHT, F(np.nan), np.nextafter(R.MIN_WEIGHT, F(1))
    m = R.planar_map(0.5, 2, bi, d, w, False, z_min=0.0, z_max=1.0)
    assert m.state.tolist() == [[1, 1, 1, 0], [1, 0, 2, 1]]


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_distance_passes_equal_the_brute_force_transform_on_every_scene(name):
    """the windowed row + column passes are the exact Euclidean transform, clipped: integer d2 over ALL cell pairs"""
    sc = S.SCENES[name]()
    for cfg in sc.configs:
        for source in S.SOURCES[:2]:
            m = S.reference(sc, cfg, source)
            assert m.W <= 64 and m.H <= 64
            want = R.brute_force_distance(m.obstacle, sc.voxel_size, cfg.get("max_distance_m", 2.0))
            assert R.same(m.distance, want), (name, cfg, source)
            assert (m.distance[m.obstacle] == 0).all()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scenes_do_not_pass_on_nothing(name):
    sc = S.SCENES[name]()
    assert len(np.unique(sc.bi, axis=0)) == len(sc.bi)
    states, zblocks, between = S.census(sc)
    print(name, "states", states, "z blocks", zblocks, "between", between)
    assert states == ("states" in sc.means), name
    assert (zblocks >= 2) == ("zblocks" in sc.means), name
    assert between == ("between" in sc.means), name


def test_the_planted_cases_land_where_the_scenes_say():
    for vps in (8, 16):
        sc = S.SCENES[f"special_vps{vps}"]()
        m = S.reference(sc, sc.configs[0], "tsdf")
        cell = lambda x, y: (y - m.y0, x - m.x0)                                  # noqa: E731
        assert R.same(m.clearance[cell(0, 0)], F(-0.0)) and R.same(m.clearance[cell(1, 0)], F(0.0))
        assert m.state[cell(0, 0)] == m.state[cell(1, 0)] == 2
        assert [int(m.state[cell(x, 0)]) for x in range(2, 8)] == [0, 1, 2, 1, 0, 0]
        assert m.clearance[cell(4, 0)] == -np.inf and m.clearance[cell(5, 0)] == np.inf
        assert m.state[cell(0, 1)] == 2 and m.state[cell(1, 1)] == 2 and m.state[cell(2, 1)] == 1
        assert m.n_occ[cell(3, 1)] == 2 and m.height[cell(3, 1)] == F(4.5 * 0.125) and m.clearance[cell(3, 1)] == F(-0.25)
        assert S.reference(sc, sc.configs[1], "tsdf").state[cell(1, 1)] == 0       # min_weight = 0.5
        e = S.reference(sc, sc.configs[0], "esdf")
        assert e.state[cell(6, 0)] == e.state[cell(7, 0)] == 0
    sc = S.SCENES["free_count"]()
    a, b, c = (S.reference(sc, cfg, "esdf") for cfg in sc.configs)
    assert a.counts[1] > b.counts[1] > 0 and c.counts[1] == 0 and (a.n_free.max(), a.n_free[a.state == 1].min()) == (3, 1)
    sc = S.SCENES["narrow"]()
    for cfg in sc.configs:
        m = S.reference(sc, cfg, "esdf")
        assert m.counts[1] == m.counts[2] == 0 and m.W * m.H == (0 if not cfg.get("use_box") else cfg["cell_dim"][0] * cfg["cell_dim"][1])
    sc = S.SCENES["gap_vps16"]()
    m = S.reference(sc, sc.configs[0], "esdf")
    col = m.z_blocks[0:16, 0:16]                                                  # the column with the missing middle block
    assert m.x0 == -48 and m.y0 == -32 and col.max() == 2 and m.z_blocks.max() == 3


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
    cfg = capi.planar_map_config()
    assert np.isnan(cfg.z_min) and np.isnan(cfg.z_max)
    assert (cfg.occupied_distance, cfg.min_free_voxels, cfg.unknown_is_obstacle, cfg.max_distance_m, cfg.use_box) == (0.0, 1, 0, 2.0, 0)
    assert F(cfg.min_weight) == R.MIN_WEIGHT and list(cfg.cell_min) + list(cfg.cell_dim) == [0, 0, 0, 0]
    cfg = capi.planar_map_config(z_min=0.1, z_max=0.5, cell_min=(-3, 4), cell_dim=(5, 6), use_box=1)
    assert list(cfg.cell_min) == [-3, 4] and list(cfg.cell_dim) == [5, 6]
    assert "vgx_planar_map_config" in text and re.search(r"typedef struct vgx_planar_map_s\* vgx_planar_map;", text)
