"""The elevation map's numpy restatement (tests/elevation_map_ref.py) against grids written out by hand, its step window
and its distance passes against brute force, the scenes of the GPU tests checked not to pass on nothing, and the new
symbols exported by libvoxgraph_amd.so and declared in include/voxgraph_amd.h."""
import os
import re

import numpy as np
import pytest

from tests import elevation_map_ref as R
from tests import elevation_map_scenes as S

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vgx_elevation_map_config_default", "vgx_elevation_map_create", "vgx_elevation_map_destroy", "vgx_tsdf_layer_elevation_map",
           "vgx_submap_layer_elevation_map", "vgx_elevation_map_stats", "vgx_elevation_map_set_timing", "vgx_elevation_map_pass_ms",
           "vgx_elevation_map_download", "vgx_elevation_map_device_pointers"]


def _columns(cols, vps=4, vs=0.5):
    """one block column of two z blocks (vps 4: 8 rows, centres 0.25, 0.75, ... 3.75) holding the given columns of 8
    distances, bottom row first, along x at y = 0; every other voxel unobserved"""
    bi = np.array([[0, 0, 0], [0, 0, 1]], np.int32)
    d = np.zeros((2, vps ** 3), F)
    o = np.zeros((2, vps ** 3), np.uint8)
    for x, col in enumerate(cols):
        for z, v in enumerate(col):
            if v is None:
                continue
            d[z // vps, x + vps * vps * (z % vps)] = v
            o[z // vps, x + vps * vps * (z % vps)] = 1
    return bi, d, o


def test_the_restatement_on_columns_written_out_by_hand():
    n, inf, nan = None, np.inf, np.nan
    cols = [[-1.0, -0.5, -0.25, 0.75, 1.0, 1.5, n, n],         # x = 0: a crossing between rows 2 and 3; t = 0.25, h = 1.25 + 0.125
            [-0.5, 0.5, -0.5, -0.5, 0.25, 0.75, 1.0, 1.0],     # x = 1: two crossings (rows 3|4 across the z blocks, and 0|1)
            [0.5, 0.5, 0.5, n, n, n, n, n],                    # x = 2: free only: a hole
            [-0.5, n, 0.5, 0.5, n, n, nan, -inf]]              # x = 3: solid and free never adjacent: blocked
    bi, d, o = _columns(cols)
    m = R.elevation_map(0.5, 4, bi, d, o, True, z_min=0.0, z_max=4.0, max_distance_m=1.0, max_slope=10.0, max_step_m=10.0)
    assert (m.x0, m.y0, m.W, m.H, m.R) == (0, 0, 4, 4, 2)
    assert m.state[0].tolist() == [1, 1, 2, 3] and not m.state[1:].any() and m.state_counts == (12, 2, 1, 1)
    # x = 0: t = 0.25 / (0.75 + 0.25); x = 1, the highest: solid row 3 (centre 1.75), t = 0.5 / 0.75
    t1 = F(0.5) / F(0.75)
    assert R.same(m.height[0], np.array([F(1.25) + F(0.25) * F(0.5), F(1.75) + t1 * F(0.5), 0, 0], F))
    assert m.headroom[0].tolist() == [3, 4, 0, 0] and m.crossings[0].tolist() == [1, 2, 0, 0]
    assert m.n_free[0].tolist() == [3, 5, 3, 2] and m.n_solid[0].tolist() == [3, 3, 0, 2]
    # step and support over the window of radius 1: the two surface cells see each other
    step = m.height[0, 1] - m.height[0, 0]
    assert R.same(m.step[0], np.array([step, step, 0, 0], F)) and m.support[0].tolist() == [2, 2, 0, 0]
    # gradient: x has one neighbour each (one-sided, / voxel_size); y has none: the slope is undefined -> class 0
    assert not m.slope_valid.any() and not R.bits(m.grad).any() and not R.bits(m.slope).any()
    assert m.cls[0].tolist() == [0, 0, 2, 2] and m.class_counts == (14, 0, 2)
    r2 = F(np.sqrt(F(2))) * F(0.5)
    assert R.same(m.distance[:2], np.array([[1.0, 0.5, 0.0, 0.0], [1.0, r2, 0.5, 0.5]], F))
    # the lowest crossing of x = 1: solid row 0 (centre 0.25), t = 0.5 / 1.0, one free voxel above it
    m = R.elevation_map(0.5, 4, bi, d, o, True, z_min=0.0, z_max=4.0, pick=1)
    assert m.height[0, 1] == F(0.5) and m.headroom[0, 1] == 1 and m.height[0, 0] == F(1.375)
    # a hole is not an obstacle when told so; the band that cuts the upper voxel of x = 0's crossing leaves it blocked
    m = R.elevation_map(0.5, 4, bi, d, o, True, z_min=0.0, z_max=1.5, hole_is_obstacle=0)
    assert m.state[0].tolist() == [3, 1, 2, 3] and m.cls[0].tolist() == [2, 0, 0, 2]


def test_gradient_slope_and_class_order_on_a_grid_written_out_by_hand():
    """a 3 x 3 patch of surface cells (one block, vps 4, voxel 0.5) with a hole in a corner: every neighbour count"""
    vs, vps = 0.5, 4
    heights = np.array([[0.5, 0.6, 0.7], [0.6, 0.8, 1.1], [0.7, 1.0, np.nan]])       # [y][x]; NaN: no surface there
    bi = np.array([[0, 0, 0]], np.int32)
    d = np.zeros((1, 64), F)
    o = np.zeros((1, 64), np.uint8)
    for y in range(3):
        for x in range(3):
            if np.isnan(heights[y, x]):
                continue
            for z in range(4):
                d[0, x + 4 * y + 16 * z] = (z + 0.5) * vs - heights[y, x]
                o[0, x + 4 * y + 16 * z] = 1
    m = R.elevation_map(vs, vps, bi, d, o, True, z_min=0.0, z_max=2.0, max_slope=0.45, max_step_m=0.35, step_radius_cells=1)
    h = m.height
    assert m.state[:3, :3].tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 0]] and np.allclose(h[:3, :3][m.state[:3, :3] == 1],
                                                                                       heights[~np.isnan(heights)], atol=1e-6)
    two = F(2.0) * F(vs)
    # the centre: both neighbours on both axes; a corner: one on each; (2, 1) [y = 1, x = 2]: its y + 1 neighbour is no surface
    assert R.same(m.grad[1, 1], np.array([(h[1, 2] - h[1, 0]) / two, (h[2, 1] - h[0, 1]) / two], F))
    assert R.same(m.grad[0, 0], np.array([(h[0, 1] - h[0, 0]) / F(vs), (h[1, 0] - h[0, 0]) / F(vs)], F))
    assert R.same(m.grad[1, 2], np.array([(h[1, 2] - h[1, 1]) / F(vs), (h[1, 2] - h[0, 2]) / F(vs)], F))
    assert R.same(m.grad[2, 1], np.array([(h[2, 1] - h[2, 0]) / F(vs), (h[2, 1] - h[1, 1]) / F(vs)], F))
    assert m.slope_valid[:3, :3].tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 0]]
    assert R.same(m.slope[1, 1], np.sqrt(m.grad[1, 1, 0] * m.grad[1, 1, 0] + m.grad[1, 1, 1] * m.grad[1, 1, 1]))
    assert m.support[:3, :3].tolist() == [[4, 6, 4], [6, 8, 5], [4, 5, 0]]
    assert R.same(m.step[1, 1], h[1, 2] - h[0, 0]) and R.same(m.step[0, 0], h[1, 1] - h[0, 0])
    # classes: slope > 0.45 or step > 0.35 -> 2
    slope_bad = m.slope[:3, :3] > F(0.45)
    step_bad = m.step[:3, :3] > F(0.35)
    want = np.where(m.state[:3, :3] == 1, np.where(slope_bad | step_bad, 2, 1), 0)
    assert m.cls[:3, :3].tolist() == want.tolist() and {0, 1, 2} <= set(m.cls[:3, :3].ravel().tolist())
    # the order: too little support gives 0 even where the step is too large; too little headroom gives 2 before either
    m2 = R.elevation_map(vs, vps, bi, d, o, True, z_min=0.0, z_max=2.0, max_slope=0.45, max_step_m=0.35, min_support=7)
    assert m2.cls[1, 1] == 2 and step_bad[1, 2] and m2.cls[1, 2] == 0
    m3 = R.elevation_map(vs, vps, bi, d, o, True, z_min=0.0, z_max=2.0, max_slope=0.45, max_step_m=0.35, min_support=7,
                         min_headroom_voxels=3)
    assert m3.headroom[1, 2] == 2 and m3.cls[1, 2] == 2 and m3.headroom[0, 0] == 3 and m3.cls[0, 0] == 0


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_step_and_distance_equal_brute_force_on_every_scene(name):
    """the separable window is the window; the windowed row + column passes are the exact Euclidean transform, clipped"""
    sc = S.SCENES[name]()
    for cfg in sc.configs:
        for source in S.SOURCES[:2]:
            m = S.reference(sc, cfg, source)
            assert m.W <= 64 and m.H <= 64
            step, support = R.brute_force_step(m.state == 1, m.height, cfg.get("step_radius_cells", 1))
            assert R.same(m.step, step) and R.same(m.support, support), (name, cfg, source)
            want = R.brute_force_distance(m.obstacle, sc.voxel_size, cfg.get("max_distance_m", 2.0))
            assert R.same(m.distance, want), (name, cfg, source)
            assert (m.distance[m.obstacle] == 0).all()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scenes_do_not_pass_on_nothing(name):
    sc = S.SCENES[name]()
    assert len(np.unique(sc.bi, axis=0)) == len(sc.bi) and len(sc.bi) <= 60
    shown = S.census(sc)
    print(name, shown)
    for what in S.ALL:
        assert shown[what] == (what in sc.means), (name, what)


def _branches(m, cfg):
    """which of the class rule's branches the cells of a map take, in the rule's order"""
    s = m.state
    low = (s == 1) & (m.headroom < cfg.get("min_headroom_voxels", 1))
    unsure = (s == 1) & ~low & ((m.slope_valid == 0) | (m.support < cfg.get("min_support", 1)))
    bad = (s == 1) & ~low & ~unsure & ((m.slope > F(cfg.get("max_slope", 1.0))) | (m.step > F(cfg.get("max_step_m", 0.2))))
    return {"unknown": s == 0, "blocked": s == 3, "hole": s == 2, "low": low, "unsure": unsure, "bad": bad, "good": (s == 1) & ~low & ~unsure & ~bad}


def test_the_planted_cases_land_where_the_scenes_say():
    for vps in (8, 16):
        sc = S.SCENES[f"special_vps{vps}"]()
        m = S.reference(sc, sc.configs[0], "tsdf")
        cell = lambda x, y: (y - m.y0, x - m.x0)                                  # noqa: E731
        vs = F(sc.voxel_size)
        row = lambda z: F((z + 0.5) * 0.125)                                      # noqa: E731 (exact)
        assert [float(m.t[cell(x, 0)]) for x in range(5)] == [0.5, 0.0, 0.5, 0.0, 0.0]
        assert R.same(m.height[cell(0, 0)], row(3) + F(0.5) * vs) and R.same(m.height[cell(1, 0)], row(3))
        assert m.state[cell(5, 0)] == 3 and m.state[cell(6, 0)] == 3      # a NaN on either side of the pair: the run is reset, no crossing
        assert m.state[cell(7, 0)] == 3                                   # a NaN weight on the free voxel: not observed, the same
        assert m.state[cell(0, 1)] == 3 and m.state[cell(1, 1)] == 1                     # weight at, and just above, the threshold
        assert m.state[cell(2, 1)] == 1 and S.reference(sc, sc.configs[2], "tsdf").state[cell(2, 1)] == 3   # min_weight = 0.5: rows 0, 1 stay
        assert m.t[cell(3, 1)] == F(0.5) and m.t[cell(4, 1)] == F(0.0)
        assert m.crossings[cell(5, 1)] == 4 and S.reference(sc, sc.configs[1], "tsdf").height[cell(5, 1)] < m.height[cell(5, 1)]
        e = S.reference(sc, sc.configs[0], "esdf")
        assert e.state[cell(7, 0)] == 3 and e.state[cell(0, 1)] == 3                      # the ESDF's observed byte decides there
    sc = S.SCENES["gap"]()
    m = S.reference(sc, sc.configs[0], "esdf")
    assert (m.state[0:8, 8:16] == 3).all() and (np.delete(m.state, np.s_[8:16], 1) == 1).all()   # the column with the missing block
    sc = S.SCENES["band"]()
    counts = [S.reference(sc, cfg, "esdf").state_counts for cfg in sc.configs]
    assert [c.index(max(c)) for c in counts[:6]] == [1, 3, 2, 3, 2, 1] and counts[6] == (0, 0, 0, 0) and counts[7] == (42, 0, 0, 0)
    for name in ("table_vps8", "table_vps16"):
        sc = S.SCENES[name]()
        hi, lo, low_room = (S.reference(sc, cfg, "tsdf") for cfg in sc.configs[:3])
        under = hi.n_cross >= 2
        assert under.sum() > 100 and (hi.height[under] > lo.height[under]).all() and R.same(hi.height[~under], lo.height[~under])
        assert (lo.headroom[under] < lo.headroom[~under].min()).all() and (low_room.cls[under] == 2).all()
        assert (S.reference(sc, sc.configs[5], "tsdf").n_cross <= 1).all()
    # every branch of the class rule is taken somewhere, and where two of them disagree the earlier one wins
    sc = S.SCENES["class_order"]()
    taken = set()
    for cfg in sc.configs:
        m = S.reference(sc, cfg, "tsdf")
        b = _branches(m, cfg)
        taken |= {k for k, v in b.items() if v.any()}
        for k, c in (("unknown", 0), ("blocked", 2), ("low", 2), ("unsure", 0), ("bad", 2), ("good", 1)):
            assert (m.cls[b[k]] == c).all(), (cfg, k)
    sc = S.SCENES["tilted_vps8"]()
    for cfg in sc.configs:
        taken |= {k for k, v in _branches(S.reference(sc, cfg, "tsdf"), cfg).items() if v.any()}
    assert taken == {"unknown", "blocked", "hole", "low", "unsure", "bad", "good"}, taken
    m = S.reference(S.SCENES["class_order"](), S.SCENES["class_order"]().configs[1], "tsdf")
    assert ((m.headroom < 3) & (m.state == 1) & (m.slope_valid == 0)).any()              # low headroom AND an undefined slope: 2
    assert ((m.state == 1) & (m.headroom >= 3) & (m.slope_valid == 0) & (m.step > F(0.3))).any()   # undefined AND a large step: 0
    # the sparse scene: no, one and two valid neighbours on an axis
    sc = S.SCENES["sparse"]()
    m = S.reference(sc, sc.configs[0], "esdf")
    s = m.state == 1
    nx = R._shift(s, 0, 1, False).astype(int) + R._shift(s, 0, -1, False)
    ny = R._shift(s, 1, 0, False).astype(int) + R._shift(s, -1, 0, False)
    assert {(int(a), int(b)) for a, b in zip(nx[s], ny[s])} == {(a, b) for a in range(3) for b in range(3)}
    assert m.slope_valid[s].tolist() == ((nx[s] > 0) & (ny[s] > 0)).astype(int).tolist()


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
    cfg = capi.elevation_map_config()
    assert np.isnan(cfg.z_min) and np.isnan(cfg.z_max)
    assert (cfg.min_free_voxels, cfg.pick, cfg.step_radius_cells, cfg.min_support, cfg.max_slope, F(cfg.max_step_m), cfg.min_headroom_voxels,
            cfg.hole_is_obstacle, cfg.unknown_is_obstacle, cfg.max_distance_m, cfg.use_box) == (1, 0, 1, 1, 1.0, F(0.2), 1, 1, 0, 2.0, 0)
    assert F(cfg.min_weight) == R.MIN_WEIGHT and list(cfg.cell_min) + list(cfg.cell_dim) == [0, 0, 0, 0]
    cfg = capi.elevation_map_config(z_min=0.1, z_max=0.5, cell_min=(-3, 4), cell_dim=(5, 6), use_box=1)
    assert list(cfg.cell_min) == [-3, 4] and list(cfg.cell_dim) == [5, 6]
    assert "vgx_elevation_map_config" in text and re.search(r"typedef struct vgx_elevation_map_s\* vgx_elevation_map;", text)
