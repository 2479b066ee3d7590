"""Voxel colours from the submap through the projected map / transformLayer into the mesh and its consumers, on the device:
bit for bit against the numpy restatement of tests/map_colour_ref.py."""
import types

import numpy as np
import pytest

from oracle import synth
from tests import map_colour_ref as mc
from tests import map_msg_ref as mm
from tests import mesh_marker_ref as mk
from tests import mesh_ref as mr
from tests import projected_map_ref as pm
from tests.test_mesh_cpu import edge_case_layer
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
IDENT = np.array([1, 0, 0, 0, 0, 0, 0], F)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _yaw_pose(yaw, t):
    return np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)


def _submap(rng, vps, vs, block_min, block_dims, coloured=True, w_scale=1.0, zero_frac=0.04, density=1.0):
    """four distinct bytes per voxel; planted 0 / 255 neighbourhoods (a slab of voxels whose bytes are all 0 or 255)"""
    bi = synth.dense_block_index(block_min, block_dims)
    if density < 1.0:
        bi = bi[rng.random(len(bi)) < density]
    n, nv = len(bi), vps ** 3
    d = rng.uniform(-0.3, 0.3, (n, nv)).astype(F)
    w = (rng.uniform(0.5, 30, (n, nv)) * w_scale).astype(F)
    w[rng.random(w.shape) < zero_frac] = 0
    rgba = None
    if coloured:
        rgba = rng.integers(0, 256, (n, nv, 4), dtype=np.uint8)
        slab = rng.random((n, nv)) < 0.3
        rgba[slab] = rng.choice(np.array([0, 255], np.uint8), (int(slab.sum()), 4))
    return types.SimpleNamespace(voxel_size=float(F(vs)), vps=vps, block_index=np.ascontiguousarray(bi, np.int32),
                                 tsdf_distance=d, tsdf_weight=w, tsdf_rgba=rgba)


def _upload(ctx, sm, sid, coloured=None):
    h = capi.Submap(ctx, sid, sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight)
    if sm.tsdf_rgba is not None and coloured is not False:
        h.set_colors(sm.tsdf_rgba)
    return h


def _as_dict(layer):
    bi, d, w, rgba = layer.download()
    return {tuple(int(v) for v in b): (dd, ww, cc) for b, dd, ww, cc in zip(bi, d, w, rgba)}


def _assert_layers_equal(got, want):
    assert set(got) == set(want), (len(set(got) ^ set(want)), sorted(set(got) ^ set(want))[:5])
    for k in want:
        for name, g, w in zip(("distance", "weight", "rgba"), got[k], want[k]):
            assert same(g, w), (k, name, np.flatnonzero(np.asarray(g).ravel() != np.asarray(w).ravel())[:5])


# ---- submap colours ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vps", [8, 16])
def test_submap_colours_round_trip_and_refusals(ctx, vps):
    rng = np.random.default_rng(vps)
    sm = _submap(rng, vps, 0.1, (-1, 0, -1), (2, 2, 2))
    h = _upload(ctx, sm, 1, coloured=False)
    assert not h.has_colors()                                               # a submap made by today's calls
    with pytest.raises(capi.VgxError) as e:
        h.download_colors()
    assert e.value.code == -1
    with pytest.raises(capi.VgxError) as e:
        h.set_colors(None)
    assert e.value.code == -1 and not h.has_colors()
    h.set_colors(sm.tsdf_rgba)
    assert h.has_colors() and same(h.download_colors(), sm.tsdf_rgba)
    again = np.ascontiguousarray(sm.tsdf_rgba[::-1])
    h.set_colors(again)                                                     # replaced in place
    assert same(h.download_colors(), again)
    with pytest.raises(capi.VgxError):
        h.set_colors(None)
    assert same(h.download_colors(), again)                                 # a refusal leaves the handle as it was
    h.release_raw_layers()
    assert not h.has_colors()
    with pytest.raises(capi.VgxError) as e:
        h.set_colors(sm.tsdf_rgba)
    assert e.value.code == -1 and not h.has_colors()
    h.destroy()


@pytest.mark.parametrize("vps", [8, 16])
def test_from_tsdf_layer_colored_copies_the_layer_colours(ctx, vps):
    rng = np.random.default_rng(10 + vps)
    sm = _submap(rng, vps, 0.1, (-2, -1, 0), (3, 2, 2))
    layer = capi.TsdfLayer(ctx, sm.voxel_size, vps)
    layer.upload(sm.block_index, sm.tsdf_distance, sm.tsdf_weight, sm.tsdf_rgba)
    lbi, _, _, lrgba = layer.download()
    h = capi.Submap.from_tsdf_layer_colored(ctx, layer, 3)
    plain = capi.Submap.from_tsdf_layer(ctx, layer, 4)
    assert h.has_colors() and not plain.has_colors()
    row = {tuple(int(c) for c in b): i for i, b in enumerate(lbi)}
    perm = [row[tuple(int(c) for c in b)] for b in h.block_index()]          # the submap's block order
    assert same(h.download_colors(), lrgba[perm])
    assert same(layer.download()[3], lrgba)                                 # the layer is left untouched
    empty = capi.TsdfLayer(ctx, sm.voxel_size, vps)
    he = capi.Submap.from_tsdf_layer_colored(ctx, empty, 5)
    assert he.has_colors() and he.download_colors().shape == (0, vps ** 3, 4)
    for x in (h, plain, he, layer, empty):
        x.destroy()


# ---- projected map -----------------------------------------------------------------------------------------------

def _merge_scene(vps):
    """three coloured submaps and one colourless; weights of 0 and 1 six orders of magnitude apart; identity, a
    grid-aligned shift, a yaw plus an off-grid offset; the colourless one reaches blocks of its own"""
    rng = np.random.default_rng(100 + vps)
    vs = 0.1 if vps == 16 else 0.2
    subs = [_submap(rng, vps, vs, (-1, -1, -1), (2, 2, 2), w_scale=1e-3),
            _submap(rng, vps, vs, (-1, -1, -1), (3, 2, 2), w_scale=1e3),
            _submap(rng, vps, vs, (-2, -1, -1), (3, 3, 2)),
            _submap(rng, vps, vs, (0, -1, -1), (4, 2, 2), coloured=False)]
    T = np.stack([IDENT, np.array([1, 0, 0, 0, 3 * vs, -2 * vs, vs], F), _yaw_pose(0.4, (0.37 * vs * 10, -0.021, 0.05)),
                  _yaw_pose(-0.2, (0.13, 0.02, -0.03))])
    return subs, T


@pytest.fixture(scope="module", params=[8, 16])
def merge_case(request):
    """the scene and its restatement, computed once: into an empty layer and into a layer that holds coloured voxels"""
    vps = request.param
    subs, T = _merge_scene(vps)
    rng = np.random.default_rng(7)
    base_bi = synth.dense_block_index((-1, -1, -1), (5, 2, 2))
    nv = vps ** 3
    bd = rng.uniform(-0.3, 0.3, (len(base_bi), nv)).astype(F)
    bw = rng.uniform(0, 8, (len(base_bi), nv)).astype(F)
    bw[:, ::5] = 0
    brgba = rng.integers(0, 256, (len(base_bi), nv, 4), dtype=np.uint8)
    want_empty = mc.merge_submaps({}, subs, T)
    want_base = mc.merge_submaps(mc.layer_from_arrays(base_bi, bd, bw, brgba), subs, T)
    alone = [mc.merge_submaps({}, [s], [t]) for s, t in zip(subs, T)]
    return types.SimpleNamespace(vps=vps, subs=subs, T=T, base=(base_bi, bd, bw, brgba), want_empty=want_empty,
                                 want_base=want_base, alone=alone)


def test_merge_into_empty_layer(ctx, merge_case):
    m = merge_case
    handles = [_upload(ctx, s, i) for i, s in enumerate(m.subs)]
    layer = capi.TsdfLayer(ctx, m.subs[0].voxel_size, m.vps)
    nb = layer.merge_submaps(handles, m.T)
    got = _as_dict(layer)
    assert nb == len(got) == len(m.want_empty) > 10
    _assert_layers_equal(got, m.want_empty)
    # colours really blended: voxels whose colour is none of the colours the submaps give on their own
    blended = 0
    for k, (_, _, c) in got.items():
        reach = [a[k][2] for a in m.alone[:3] if k in a]
        if len(reach) >= 2:
            blended += int(np.all([(c != r).any(1) for r in reach], 0).sum())
    assert blended > 100
    # blocks only the colourless submap reached carry no colour
    only = set(m.alone[3]) - set().union(*m.alone[:3])
    assert only and all(not got[k][2].any() for k in only)
    for h in handles:
        h.destroy()
    layer.destroy()


def test_merge_into_coloured_layer(ctx, merge_case):
    m = merge_case
    base_bi, bd, bw, brgba = m.base
    handles = [_upload(ctx, s, i) for i, s in enumerate(m.subs)]
    layer = capi.TsdfLayer(ctx, m.subs[0].voxel_size, m.vps)
    layer.upload(base_bi, bd, bw, brgba)
    layer.merge_submaps(handles, m.T)
    got = _as_dict(layer)
    _assert_layers_equal(got, m.want_base)
    base = {tuple(int(c) for c in b): i for i, b in enumerate(base_bi)}
    only = (set(m.alone[3]) - set().union(*m.alone[:3])) & set(base)
    assert only and all(same(got[k][2], brgba[base[k]]) for k in only)      # they keep their bytes
    touched = [k for k in base if k in set().union(*m.alone[:3])]
    assert any(not same(got[k][2], brgba[base[k]]) for k in touched)
    for h in handles:
        h.destroy()
    layer.destroy()


def test_identity_pose_copies_colours_exactly(ctx, merge_case):
    m = merge_case
    sm = m.subs[2]
    h = _upload(ctx, sm, 0)
    layer = capi.TsdfLayer(ctx, sm.voxel_size, m.vps)
    layer.merge_submaps([h], IDENT[None])
    got = _as_dict(layer)
    row = {tuple(int(c) for c in b): i for i, b in enumerate(sm.block_index)}
    n_copied = 0
    for k, (d, w, c) in got.items():
        hit = w > 0                                                         # the voxels that interpolated
        assert same(c[hit], sm.tsdf_rgba[row[k]][hit]) and not c[~hit].any()
        n_copied += int(hit.sum())
    assert n_copied > 1000
    _assert_layers_equal(got, mc.merge_submaps({}, [sm], IDENT[None]))
    h.destroy()
    layer.destroy()


def test_colourless_inputs_give_todays_bytes(ctx, merge_case):
    """the guard that nothing existing moved: no submap has colours -> the projected map of tests/projected_map_ref.py,
    the layer's rgba untouched"""
    m = merge_case
    base_bi, bd, bw, brgba = m.base
    handles = [_upload(ctx, s, i, coloured=False) for i, s in enumerate(m.subs)]
    assert not any(h.has_colors() for h in handles)
    layer = capi.TsdfLayer(ctx, m.subs[0].voxel_size, m.vps)
    layer.upload(base_bi, bd, bw, brgba)
    layer.merge_submaps(handles, m.T)
    got = _as_dict(layer)
    want = pm.merge_submaps(pm.layer_from_arrays(base_bi, bd, bw), m.subs, m.T)
    assert set(got) == set(want)
    base = {tuple(int(c) for c in b): i for i, b in enumerate(base_bi)}
    for k in want:
        assert same(got[k][0], want[k][0]) and same(got[k][1], want[k][1])
        assert same(got[k][2], brgba[base[k]]) if k in base else not got[k][2].any()
    for h in handles:
        h.destroy()
    layer.destroy()


@pytest.mark.parametrize("vps", [8, 16])
def test_transform_submap_with_colours(ctx, vps):
    rng = np.random.default_rng(200 + vps)
    vs = 0.1 if vps == 16 else 0.2
    sm = _submap(rng, vps, vs, (-1, -1, 0), (3, 2, 2), zero_frac=0.1, density=0.8)
    T = _yaw_pose(0.7, (0.11, -0.07, 0.03))
    h = _upload(ctx, sm, 0)
    layer = capi.TsdfLayer(ctx, sm.voxel_size, vps)
    layer.transform_submap(h, T)
    got = _as_dict(layer)
    want = mc.transform_submap(sm, T)
    _assert_layers_equal(got, want)
    miss = np.concatenate([w == 0 for _, w, _ in got.values()])
    col = np.concatenate([c for _, _, c in got.values()])
    assert miss.any() and not col[miss].any()                               # kept blocks with voxels that did not interpolate
    assert len(np.unique(col[~miss], axis=0)) > 100
    # the same submap without colours: rgba untouched (zeros in the empty layer)
    plain = _upload(ctx, sm, 1, coloured=False)
    layer2 = capi.TsdfLayer(ctx, sm.voxel_size, vps)
    layer2.transform_submap(plain, T)
    got2 = _as_dict(layer2)
    assert set(got2) == set(got)
    assert all(same(got2[k][0], got[k][0]) and same(got2[k][1], got[k][1]) and not got2[k][2].any() for k in got)
    for x in (h, plain, layer, layer2):
        x.destroy()


# ---- mesh --------------------------------------------------------------------------------------------------------

def _mesh_scene(vps, seed, dims=(3, 2, 2)):
    rng = np.random.default_rng(seed)
    bi, d, w = edge_case_layer(rng, vps, (-1, -1, -1), dims, density=0.9)
    rgba = rng.integers(0, 256, (len(bi), vps ** 3, 4), dtype=np.uint8)
    return bi, d, w, rgba


@pytest.fixture(scope="module", params=[(8, 0), (16, 1)])
def mesh_case(request):
    vps, seed = request.param
    bi, d, w, rgba = _mesh_scene(vps, seed)
    want = mr.generate_mesh(bi, d, w, vps, 0.1, 1e-4)
    colours, moved = mc.vertex_colours(want[0], want[1], want[2], bi, w, rgba, vps, 0.1, 1e-4)
    return types.SimpleNamespace(vps=vps, bi=bi, d=d, w=w, rgba=rgba, want=want, colours=colours, moved=moved)


@pytest.mark.parametrize("source", ["layer", "submap"])
def test_vertex_colours_bit_exact(ctx, mesh_case, source):
    m = mesh_case
    if source == "layer":
        src = capi.TsdfLayer(ctx, 0.1, m.vps)
        src.upload(m.bi, m.d, m.w, m.rgba)
    else:
        src = capi.Submap(ctx, 0, 0.1, m.vps, m.bi, m.d, m.w)
        src.set_colors(m.rgba)
    plain = src.generate_mesh().download()
    mesh = src.generate_mesh_colored()
    assert mesh.color_layout() == capi.MESH_COLORS_PER_VERTEX and mesh.has_colors()
    got = mesh.download()
    for g, p, w in zip(got, plain, m.want[:4]):                             # identical to the plain generator's
        assert same(g, p) and same(g, w)
    c = mesh.download_vertex_colors()
    assert same(c, m.colours)
    assert m.moved.any()                                                    # vertices coloured from a neighbouring block
    assert len(np.unique(c.reshape(-1, 4), axis=0)) >= 100
    with pytest.raises(capi.VgxError) as e:
        mesh.download_colors()                                              # one per triangle: the size differs
    assert e.value.code == -1 and mesh.color_layout() == capi.MESH_COLORS_PER_VERTEX
    mesh.destroy()
    src.destroy()


def test_one_cube_empty_layer_and_a_reused_handle(ctx):
    vps, vs = 8, 0.1
    nv = vps ** 3
    mesh = capi.Mesh(ctx)
    # the empty layer
    empty = capi.TsdfLayer(ctx, vs, vps)
    empty.generate_mesh_colored(mesh)
    assert mesh.stats() == (0, 0) and mesh.color_layout() == capi.MESH_COLORS_PER_VERTEX
    assert mesh.download_vertex_colors().shape == (0, 3, 4)
    # one cube: one block, one negative corner
    d = np.full((1, nv), 0.2, F)
    d[0, 0] = -0.1
    w = np.ones((1, nv), F)
    rgba = np.arange(nv * 4, dtype=np.uint32).astype(np.uint8).reshape(1, nv, 4)
    bi = np.zeros((1, 3), np.int32)
    one = capi.TsdfLayer(ctx, vs, vps)
    one.upload(bi, d, w, rgba)
    one.generate_mesh_colored(mesh)
    want = mr.generate_mesh(bi, d, w, vps, vs)
    assert mesh.stats() == (1, 1) and same(mesh.download()[2], want[2])
    assert same(mesh.download_vertex_colors(), mc.vertex_colours(want[0], want[1], want[2], bi, w, rgba, vps, vs)[0])
    # large / small / large, coloured and plain in turn
    big = _mesh_scene(vps, 5)
    large = capi.TsdfLayer(ctx, vs, vps)
    large.upload(*big)
    wl = mr.generate_mesh(big[0], big[1], big[2], vps, vs)
    cl = mc.vertex_colours(wl[0], wl[1], wl[2], big[0], big[2], big[3], vps, vs)[0]
    for src, coloured in ((large, True), (one, False), (large, False), (one, True), (large, True)):
        (src.generate_mesh_colored if coloured else src.generate_mesh)(mesh)
        assert mesh.color_layout() == (capi.MESH_COLORS_PER_VERTEX if coloured else capi.MESH_COLORS_NONE)
        assert same(mesh.download()[2], wl[2] if src is large else want[2])
        if coloured:
            assert same(mesh.download_vertex_colors(), cl if src is large else
                        mc.vertex_colours(want[0], want[1], want[2], bi, w, rgba, vps, vs)[0])
        else:
            with pytest.raises(capi.VgxError):
                mesh.download_vertex_colors()
    # a separated mesh on the same handle keeps its per-triangle layout
    sm = capi.Submap(ctx, 0, vs, vps, big[0], big[1], big[2])
    mesh.generate_separated([sm], IDENT[None], np.array([[1, 2, 3, 4]], np.uint8))
    assert mesh.color_layout() == capi.MESH_COLORS_PER_TRIANGLE and mesh.download_colors().shape == (mesh.stats()[1], 4)
    with pytest.raises(capi.VgxError):
        mesh.download_vertex_colors()
    # the submap form refuses a submap without colours and leaves the handle as it was
    before = mesh.stats()
    with pytest.raises(capi.VgxError) as e:
        sm.generate_mesh_colored(mesh)
    assert e.value.code == -1 and mesh.stats() == before and mesh.color_layout() == capi.MESH_COLORS_PER_TRIANGLE
    for x in (sm, empty, one, large, mesh):
        x.destroy()


# ---- consumers ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def odd_mesh_scene():
    """the first seed whose mesh has an odd triangle count (decided on the host)"""
    for seed in range(20, 40):
        bi, d, w, rgba = _mesh_scene(8, seed, dims=(2, 2, 2))
        want = mr.generate_mesh(bi, d, w, 8, 0.1)
        if len(want[2]) % 2 == 1:
            colours = mc.vertex_colours(want[0], want[1], want[2], bi, w, rgba, 8, 0.1)[0]
            return types.SimpleNamespace(bi=bi, d=d, w=w, rgba=rgba, want=want, colours=colours)
    raise AssertionError("no odd triangle count in 20 seeds")


def _coloured_mesh(ctx, s):
    layer = capi.TsdfLayer(ctx, 0.1, 8)
    layer.upload(s.bi, s.d, s.w, s.rgba)
    mesh = layer.generate_mesh_colored()
    layer.destroy()
    return mesh


@pytest.mark.parametrize("mode", [mk.COLOR, mk.LAMBERT_COLOR])
def test_marker_per_vertex(ctx, odd_mesh_scene, mode):
    s = odd_mesh_scene
    mesh = _coloured_mesh(ctx, s)
    assert mesh.stats()[1] % 2 == 1
    marker = capi.fill_marker(mesh, color_mode=mode, opacity=0.7)
    points, colors = marker.download()
    wp, wc = mc.fill_marker(s.want[2], s.want[3], s.colours, mode, 0.7)
    assert same(points, wp) and same(colors, wc)
    # a vertex's colour is its own: triangles exist whose three vertices differ
    assert (np.abs(colors.reshape(-1, 3, 4) - colors.reshape(-1, 3, 4)[:, :1]).sum((1, 2)) > 0).any()
    # the other modes are unchanged by the layout
    for other in (mk.NORMALS, mk.HEIGHT, mk.GRAY, mk.LAMBERT):
        capi.fill_marker(mesh, color_mode=other, out=marker)
        assert same(marker.download()[1], mk.fill_marker(s.want[2], s.want[3], None, other)[1])
    marker.destroy()
    mesh.destroy()


def test_weld_takes_the_first_vertex_own_colour(ctx, odd_mesh_scene, tmp_path):
    s = odd_mesh_scene
    mesh = _coloured_mesh(ctx, s)
    for thr in (1e-10, 0.1):                # voxblox's default; a voxel: vertices of different voxels weld
        cm = mesh.connect(thr)
        got = cm.download()
        want = mc.connect(s.want[2], s.want[3], s.colours, F(thr))
        assert cm.stats()[2] and all(same(g, w) for g, w in zip(got, want))
        cm.destroy()
    # (at one voxel) a planted pair: coincident after welding, of different colours -- the first one's colour wins
    idx = want[3].ravel().astype(np.int64)
    soup_c = s.colours.reshape(-1, 4)
    first = np.full(len(want[0]), len(idx), np.int64)
    np.minimum.at(first, idx, np.arange(len(idx)))
    differs = (soup_c != soup_c[first[idx]]).any(1)
    assert differs.any() and same(want[2], soup_c[first])
    # both PLY files parsed back
    soup_ply, weld_ply = tmp_path / "soup.ply", tmp_path / "weld.ply"
    mesh.write_ply(soup_ply)
    v, f = mc.read_ply(soup_ply)
    assert same(np.stack([v["x"], v["y"], v["z"]], -1), s.want[2].reshape(-1, 3))
    assert same(np.stack([v["red"], v["green"], v["blue"], v["alpha"]], -1), soup_c)
    assert same(np.stack([v["nx"], v["ny"], v["nz"]], -1), np.repeat(s.want[3], 3, axis=0))
    assert np.array_equal(f.ravel(), np.arange(len(soup_c)))
    cm = mesh.connect(0.1)
    cm.write_ply(weld_ply)
    v, f = mc.read_ply(weld_ply)
    assert same(np.stack([v["x"], v["y"], v["z"]], -1), want[0])
    assert same(np.stack([v["red"], v["green"], v["blue"], v["alpha"]], -1), want[2])
    assert np.array_equal(f.astype(np.uint32), want[3])
    cm.destroy()
    mesh.destroy()


def test_weld_of_a_planted_coincident_pair(ctx):
    """one cube whose three vertices lie in three different voxels, hence in three colours; at a pitch of four voxels all
    three share one cell: the welded vertex takes the colour of soup vertex 0, not the triangle's other two"""
    vps, vs = 8, 0.1
    nv = vps ** 3
    d = np.full((1, nv), 0.1, F)
    d[0, 0] = -0.2                                                          # t = 2/3 on each edge: beyond voxel 0
    w = np.ones((1, nv), F)
    rgba = np.zeros((1, nv, 4), np.uint8)
    rgba[0, 1], rgba[0, vps], rgba[0, vps * vps] = (10, 20, 30, 40), (50, 60, 70, 80), (90, 100, 110, 120)
    bi = np.zeros((1, 3), np.int32)
    layer = capi.TsdfLayer(ctx, vs, vps)
    layer.upload(bi, d, w, rgba)
    mesh = layer.generate_mesh_colored()
    c = mesh.download_vertex_colors()
    assert c.shape == (1, 3, 4)
    assert sorted(map(tuple, c[0].tolist())) == [(10, 20, 30, 40), (50, 60, 70, 80), (90, 100, 110, 120)]
    cm = mesh.connect(0.4)
    v, n, wc, idx = cm.download()
    assert len(v) == 1 and idx.tolist() == [[0, 0, 0]]
    assert same(wc[0], c[0, 0]) and same(v[0], mesh.download()[2][0, 0])
    for x in (cm, mesh, layer):
        x.destroy()


@pytest.mark.parametrize("vps", [8, 16])
def test_coloured_submap_serialises_its_colour_words(ctx, vps):
    rng = np.random.default_rng(300 + vps)
    sm = _submap(rng, vps, 0.1, (0, -1, 0), (2, 2, 1))
    h = _upload(ctx, sm, 0)
    msg = h.serialize_layer("tsdf")
    bi, words = msg.download()
    assert same(bi, sm.block_index)
    assert same(words.reshape(len(bi), -1), mm.tsdf_words(sm.tsdf_distance, sm.tsdf_weight, sm.tsdf_rgba))
    plain = _upload(ctx, sm, 1, coloured=False)
    plain.serialize_layer("tsdf", msg)
    assert same(msg.download()[1].reshape(len(bi), -1), mm.tsdf_words(sm.tsdf_distance, sm.tsdf_weight, None))
    for x in (h, plain, msg):
        x.destroy()


# ---- end to end --------------------------------------------------------------------------------------------------

def _lidar_scan(seed):
    """a LiDAR-shaped scan of a box room, one colour per point"""
    rng = np.random.default_rng(seed)
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, 256, endpoint=False) + (2 * np.pi / 256) / 3.0,
                         np.linspace(-0.3, 0.3, 12) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    lo, hi = np.array([-2.0, -1.6, -0.8]), np.array([2.2, 1.8, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    pts = (d * t[:, None]).astype(F)
    rgba = rng.integers(0, 256, (len(pts), 4), dtype=np.uint8)
    return pts, rgba


def test_end_to_end_scans_to_ply(ctx, tmp_path):
    vps, vs = 16, 0.2
    poses = np.stack([np.array([1, 0, 0, 0, 0.1, -0.05, 0.02], F), _yaw_pose(0.3, (0.4, 0.1, 0.0))])
    subs, handles = [], []
    for i in range(2):
        layer = capi.TsdfLayer(ctx, vs, vps)
        integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
        pts, rgba = _lidar_scan(i)
        assert integ.integratePointCloud(IDENT, pts, rgba) > 0
        bi, d, w, c = layer.download()
        assert len(np.unique(c.reshape(-1, 4), axis=0)) > 10
        h = capi.Submap.from_tsdf_layer_colored(ctx, layer, i)
        row = {tuple(int(v) for v in b): k for k, b in enumerate(bi)}
        perm = [row[tuple(int(v) for v in b)] for b in h.block_index()]
        assert same(h.download_colors(), c[perm])
        subs.append(types.SimpleNamespace(voxel_size=float(F(vs)), vps=vps, block_index=bi[perm], tsdf_distance=d[perm],
                                          tsdf_weight=w[perm], tsdf_rgba=c[perm]))
        handles.append(h)
        integ.destroy()
        layer.destroy()
    proj = capi.TsdfLayer(ctx, vs, vps)
    mesh = capi.combined_mesh(ctx, handles, poses, proj, use_color=True)
    got = _as_dict(proj)
    want = mc.merge_submaps({}, subs, poses)
    _assert_layers_equal(got, want)
    keys = sorted(want)
    wbi = np.array(keys, np.int32)
    wd, ww, wc = (np.stack([want[k][j] for k in keys]) for j in range(3))
    wm = mr.generate_mesh(wbi, wd, ww, vps, vs)
    wcol = mc.vertex_colours(wm[0], wm[1], wm[2], wbi, ww, wc, vps, vs)[0]
    assert len(wm[2]) > 1000
    assert all(same(g, w) for g, w in zip(mesh.download(), wm[:4]))
    assert same(mesh.download_vertex_colors(), wcol)
    cm = mesh.connect(1e-10)
    wcm = mc.connect(wm[2], wm[3], wcol)
    assert all(same(g, w) for g, w in zip(cm.download(), wcm))
    path = tmp_path / "combined.ply"
    cm.write_ply(path)
    v, f = mc.read_ply(path)
    ply_c = np.stack([v["red"], v["green"], v["blue"], v["alpha"]], -1)
    assert same(ply_c, wcm[2]) and np.array_equal(f.astype(np.uint32), wcm[3])
    assert len(np.unique(ply_c, axis=0)) > 10
    for x in handles + [proj, mesh, cm]:
        x.destroy()
