"""tests/map_colour_ref.py checked by properties that do not trust it (no GPU): the restatement the device is compared
with bit for bit in tests/test_map_colour_gpu.py."""
import math
import types

import numpy as np

from tests import map_colour_ref as mc
from tests import map_msg_ref as mm
from tests import projected_map_ref as pm

F = np.float32


def full_submap(rng, vps, dims=(2, 2, 2), vs=0.1, rgba=True):
    bi = np.stack(np.meshgrid(*[np.arange(-1, -1 + d) for d in dims], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    n, nv = len(bi), vps ** 3
    return types.SimpleNamespace(
        voxel_size=vs, vps=vps, block_index=bi, tsdf_distance=rng.uniform(-0.3, 0.3, (n, nv)).astype(F),
        tsdf_weight=rng.uniform(0.5, 5, (n, nv)).astype(F),
        tsdf_rgba=rng.integers(0, 256, (n, nv, 4), dtype=np.uint8) if rgba else None)


def test_interpolating_at_a_voxel_centre_returns_that_voxel():
    rng = np.random.default_rng(0)
    for vps in (8, 16):
        sm = full_submap(rng, vps)
        raw = mc.ColourLayer(sm)
        # every voxel of block 0 whose +1 neighbours exist (the block has +x, +y, +z neighbours: it is (-1, -1, -1))
        centres = pm.block_centres(sm.block_index[:1], vps, F(sm.voxel_size))[0]
        ok, d, w, c, _ = raw.interp_coloured(centres)
        assert ok.all()
        assert np.array_equal(c, sm.tsdf_rgba[0])
        assert np.array_equal(d.view(np.uint32), sm.tsdf_distance[0].view(np.uint32))
        assert np.array_equal(w.view(np.uint32), sm.tsdf_weight[0].view(np.uint32))


def test_distance_and_weight_are_the_projected_map_restatement():
    rng = np.random.default_rng(1)
    sm = full_submap(rng, 8)
    sm.tsdf_weight[rng.random(sm.tsdf_weight.shape) < 0.05] = 0
    p = rng.uniform(-0.9, 0.9, (4000, 3)).astype(F)
    ok0, d0, w0 = pm.RawLayer(sm).interp(p)
    ok1, d1, w1, c, _ = mc.ColourLayer(sm).interp_coloured(p)
    assert np.array_equal(ok0, ok1) and ok0.any() and not ok0.all()
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    assert not c[~ok1].any()


def planted_patterns():
    """the 0 / 255 neighbourhoods of one channel: one corner against the other seven, both ways, for every corner"""
    pats = []
    for k in range(8):
        for lone, rest in ((0, 255), (255, 0)):
            x = np.full(8, rest, np.uint8)
            x[k] = lone
            pats.append(x)
    return np.array(pats)                                                    # [16][8]


def test_the_clamp_is_live_on_planted_neighbourhoods():
    pats = planted_patterns()
    # dl within a few ulps of the cube's faces, where the true interpolant touches 0 or 255
    g = np.array([0.0, 1e-7, 0.3333333, 0.5, 0.7, 0.9999999, 0.99999994], F)
    x, y, z = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    over = under = 0
    for pat in pats:
        c8 = [np.broadcast_to(np.uint8(v), x.shape + (4,)) for v in pat]
        c, raw = mc.interp_channels(c8, x, y, z)
        over += int((raw > 255).sum())
        under += int((raw < 0).sum())
        assert c.dtype == np.uint8
        assert np.array_equal(c.astype(np.float64), np.trunc(np.clip(raw.astype(np.float64), 0, 255)))
        # the exact interpolant lies in [0, 255]: the overshoot is rounding, a few ulps of 255 at most
        assert raw.max() <= 255 + 1e-3 and raw.min() >= -1e-3
        assert (c[raw > 255] == 255).all() and (c[raw < 0] == 0).all()
    assert over + under > 0, "no planted case overshoots before the clamp: the clamp would be dead"


def literal_blend(oc, color, old_w, w):
    """blended_color (vgx_tsdf_internal.h) transcribed with scalars"""
    total = F(old_w) + F(w)
    fw, sw = F(F(old_w) / total), F(F(w) / total)
    out = []
    for a, b in zip(oc, color):
        v = F(F(F(a) * fw) + F(F(b) * sw))
        out.append(int(math.floor(float(v) + 0.5)) & 255)                    # roundf (v >= 0), then the uint8_t cast
    return out


def test_blended_color_agrees_with_the_message_blend_and_a_literal_transcription():
    rng = np.random.default_rng(2)
    n = 3000
    co, cn = rng.integers(0, 256, (n, 4), dtype=np.uint8), rng.integers(0, 256, (n, 4), dtype=np.uint8)
    wo = rng.uniform(1e-3, 50, n).astype(F)
    wn = rng.uniform(1e-3, 50, n).astype(F)
    wo[:200] *= F(1e6)                                                       # six orders of magnitude apart, both ways
    wn[200:400] *= F(1e6)
    wo[400:420] = 0
    got = mc.blended_color(co, cn, wo, wn)
    assert np.array_equal(got, mm.blend(co, cn, wo, wn))
    want = np.array([literal_blend(co[i], cn[i], wo[i], wn[i]) for i in range(n)], np.uint8)
    assert np.array_equal(got, want)
    assert np.array_equal(got[400:420], cn[400:420])                         # old weight 0: the new colour


def test_nearest_voxel_puts_a_max_plane_vertex_in_the_neighbouring_block():
    for vps in (8, 16):
        vs = 0.1
        bs = float(F(F(vps) * F(vs)))
        block = np.array([[-1, 2, 0]] * 4, np.int64)
        o = block[0] * bs
        p = np.array([o + [(vps - 0.3) * vs, 0.05, 0.05],                    # inside: the last voxel on x
                      o + [(vps + 0.2) * vs, 0.05, 0.05],                    # on the max-X cubes, beyond the block
                      o + [0.05, (vps + 0.4) * vs, (vps + 0.1) * vs],        # beyond on y and z
                      o + [0.05, 0.05, 0.05]], F)
        b, v, moved = mc.nearest_voxel(p, block, vps, vs)
        assert moved.tolist() == [False, True, True, False]
        assert b.tolist() == [[-1, 2, 0], [0, 2, 0], [-1, 3, 1], [-1, 2, 0]]
        assert v.tolist() == [[vps - 1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]


def test_vertex_colours_take_the_voxel_bytes_or_the_default():
    vps, vs = 8, 0.1
    rng = np.random.default_rng(3)
    bi = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    w = np.ones((2, vps ** 3), F)
    rgba = rng.integers(1, 256, (2, vps ** 3, 4), dtype=np.uint8)
    w[1, 0] = F(1e-4)                                                        # weight == min_weight is valid here (>=)
    w[1, 1] = F(5e-5)                                                        # below: the default colour
    verts = np.array([[[0.82, 0.05, 0.05], [0.95, 0.05, 0.05], [0.05, 0.85, 0.05]]], F)   # block (0,0,0)'s triangle
    c, moved = mc.vertex_colours(bi[:1], np.array([0, 1]), verts, bi, w, rgba, vps, vs)
    assert moved.tolist() == [[True, True, True]]
    assert np.array_equal(c[0, 0], rgba[1, 0]) and not c[0, 1].any() and not c[0, 2].any()   # the last: block absent
