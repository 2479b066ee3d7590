"""Map messages without a GPU: the numpy restatement (tests/map_msg_ref.py) that the GPU tests compare the kernels with,
held against the library's existing host codec of the same block words (vgx_map_file_write / vgx_map_file_read_submap)
and against hand-computed voxels; and the new symbols in the built library and in capi.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import map_msg_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vgx_map_msg_create", "vgx_map_msg_destroy", "vgx_map_msg_stats", "vgx_map_msg_layer_geometry", "vgx_map_msg_download",
           "vgx_map_msg_device_pointers", "vgx_tsdf_layer_serialize", "vgx_submap_serialize_layer", "vgx_submap_surface_msg",
           "vgx_tsdf_layer_deserialize", "vgx_tsdf_layer_deserialize_msg"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from voxgraph_amd import capi as m
    m.load()
    return m


def test_symbols_and_constants_are_in_the_library_and_in_capi(capi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    for name in SYMBOLS:
        assert name in exported and name in capi.SIGNATURES and re.search(r"VGX_API int %s\(" % name, header), name
    # voxblox MapDerializationAction [recalled]: kUpdate, kMerge, kReset
    assert (capi.MSG_ACTION_UPDATE, capi.MSG_ACTION_MERGE, capi.MSG_ACTION_RESET) == (R.UPDATE, R.MERGE, R.RESET) == (0, 1, 2)
    for name, value in (("VGX_MSG_ACTION_UPDATE", 0), ("VGX_MSG_ACTION_MERGE", 1), ("VGX_MSG_ACTION_RESET", 2), ("VGX_MSG_NONE", 0),
                        ("VGX_MSG_TSDF_LAYER", capi.MSG_TSDF_LAYER), ("VGX_MSG_ESDF_LAYER", capi.MSG_ESDF_LAYER),
                        ("VGX_MSG_SURFACE_CLOUD", capi.MSG_SURFACE_CLOUD)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert all(hasattr(capi, n) for n in ("MapMsg", "surface_msg_layout")) and hasattr(capi.TsdfLayer, "serialize")
    assert all(hasattr(capi.TsdfLayer, n) for n in ("deserialize", "deserialize_msg"))
    assert all(hasattr(capi.Submap, n) for n in ("serialize_layer", "surface_msg"))
    lay = capi.surface_msg_layout(7)
    assert (lay.width, lay.height, lay.point_step, lay.row_step, lay.offset_x, lay.offset_y, lay.offset_z, lay.color_kind,
            lay.color_offset, lay.is_bigendian) == (7, 1, 32, 224, 0, 4, 8, capi.SCAN_COLOR_INTENSITY, 16, 0)
    assert capi.scan_layout_check(lay, 224) == capi.OK and capi.scan_layout_check(lay, 223) == capi.ERR_INVALID
    # NULL handles are refused without a device
    lib = capi.load()
    assert lib.vgx_map_msg_destroy(None) == capi.ERR_INVALID and lib.vgx_map_msg_stats(None, None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_tsdf_layer_deserialize_msg(None, 0, None) == capi.ERR_INVALID


def test_words_per_voxel_follow_the_schema_table():
    src = open(os.path.join(ROOT, "voxgraph_amd", "csrc", "vgx_mapfile_schema.h")).read()
    k = {a: int(b) for a, b in re.findall(r"constexpr int (k\w+) = (\d+);", src)}
    assert (k["kTsdfWordsPerVoxel"], k["kEsdfWordsPerVoxel"]) == (R.TSDF_WORDS, R.ESDF_WORDS)


def _varints(words):
    out = bytearray()
    for v in words:
        v = int(v)
        while v >= 0x80:
            out.append((v & 0x7f) | 0x80)
            v >>= 7
        out.append(v)
    return bytes(out)


@pytest.mark.parametrize("vps", [8, 16])
def test_restatement_against_the_host_codec(capi, tmp_path, vps):
    """what vgx_map_file_write emits for a layer IS the restatement's words (found in the file as the packed varints of
    voxel_data), and what vgx_map_file_read_submap reads back is the restatement's decode of its own encode"""
    rng = np.random.default_rng(vps)
    nb, nv = 3, vps ** 3
    bi = np.array([[40, -46, 43], [-2, 0, 1], [0, 0, 0]], np.int32)
    d = rng.normal(0, 0.2, (nb, nv)).astype(F)
    w = rng.uniform(0, 10, (nb, nv)).astype(F)
    d[0, :4] = [np.nan, np.inf, -np.inf, -0.0]
    w[0, 4:6] = [0.0, -0.0]
    rgba = rng.integers(0, 256, (nb, nv, 4)).astype(np.uint8)
    rgba[0, 0] = [1, 2, 3, 4]                                   # four distinct bytes: the order shows
    ed = rng.normal(0, 1, (nb, nv)).astype(F)
    eo = (rng.random((nb, nv)) < 0.7).astype(np.uint8)
    eo[0, :3] = [200, 0, 1]                                     # observed is "!= 0" and is written as 1
    tw, ew = R.tsdf_words(d, w, rgba), R.esdf_words(ed, eo)
    assert tw.shape == (nb, nv * 3) and ew.shape == (nb, nv * 2) and tw.dtype == ew.dtype == np.uint32
    assert tw[0, 2] == 4 | 3 << 8 | 2 << 16 | 1 << 24 and ew[0, 1::2][:3].tolist() == [1, 0, 1]
    sub = dict(id=5, block_index=bi, tsdf_distance=d, tsdf_weight=w, tsdf_rgba=rgba, esdf_distance=ed, esdf_observed=eo)
    path = str(tmp_path / "m.cblox")
    capi.write_map_file(path, capi.FILE_CBLOX_COLLECTION, 0.1, vps, [sub])
    raw = open(path, "rb").read()
    for b in range(nb):
        assert _varints(tw[b]) in raw and _varints(ew[b]) in raw, b
    got = capi.MapFile(path).read_submap(0, True)
    dd, dw, dc = R.tsdf_decode(tw)
    xd, xo = R.esdf_decode(ew)
    assert R.same(got["tsdf_distance"], dd) and R.same(got["tsdf_weight"], dw) and R.same(got["tsdf_rgba"], dc)
    assert R.same(got["esdf_distance"], xd) and R.same(got["esdf_observed"], xo)
    assert R.same(dd, d) and R.same(dw, w) and R.same(dc, rgba) and R.same(xd, ed) and R.same(xo, (eo != 0).astype(np.uint8))
    # a submap's TSDF layer has no colours: word 2 is 0
    assert not R.tsdf_words(d, w)[:, 2::3].any()
    assert R.same(R.colour_bytes(R.colour_word(rgba)), rgba)


def test_merge_against_hand_computed_voxels():
    """mergeVoxelAIntoVoxelB(A = message, B = layer) and blended_color(B.colour, A.colour, wB, wA), worked by hand"""
    cA, cB = [200, 100, 0, 255], [100, 50, 7, 0]
    # wA = 1, wB = 3: d = (2 * 1 + (-2) * 3) / 4 = -1; colour = B * 0.75 + A * 0.25 = (125, 62.5 -> 63, 5.25 -> 5, 63.75 -> 64)
    d, w, c = R.merge_voxels(F(2), F(1), cA, F(-2), F(3), cB)
    assert (float(d), float(w), c.tolist()) == (-1.0, 4.0, [125, 63, 5, 64])
    # w' = 0: unchanged, bit for bit (B's -0.0 distance stays -0.0)
    d, w, c = R.merge_voxels(F(2), F(0), cA, F(-0.0), F(0), cB)
    assert (d.view(np.uint32), float(w), c.tolist()) == (0x80000000, 0.0, cB)
    # the message voxel has weight 0, the layer's 2: d = (5 * 0 + 0.3 * 2) / 2 in f32, colour B
    d, w, c = R.merge_voxels(F(5), F(0), cA, F(0.3), F(2), cB)
    assert (d, float(w), c.tolist()) == ((F(5) * F(0) + F(0.3) * F(2)) / F(2), 2.0, cB)
    # the layer voxel has weight 0: the message's voxel, (d * w) / w need not be d but here is; colour A
    d, w, c = R.merge_voxels(F(0.25), F(1.5), cA, F(9), F(0), cB)
    assert (float(d), float(w), c.tolist()) == (0.25, 1.5, cA)
    # a NaN sum is not > 0: unchanged
    d, w, c = R.merge_voxels(F(1), F(np.nan), cA, F(0.5), F(1), cB)
    assert (float(d), float(w), c.tolist()) == (0.5, 1.0, cB)
    # f32 and the association: (dA * wA + dB * wB) / w', one rounding each
    dA, wA, dB, wB = F(0.1), F(0.3), F(-0.7), F(1.1)
    d, w, _ = R.merge_voxels(dA, wA, cA, dB, wB, cB)
    assert d == F(F(F(dA * wA) + F(dB * wB)) / F(wA + wB)) and w == F(wA + wB)
    # roundf is half away from zero: 0.5 * 1 + 0.5 * 2 = 1.5 -> 2, 0.5 * 2 + 0.5 * 3 = 2.5 -> 3 (np.round would give 2, 2)
    assert R.blend([1, 2, 0, 0], [2, 3, 0, 0], F(1), F(1)).tolist() == [2, 3, 0, 0]


def test_actions_on_a_small_layer():
    nv = 8
    layer = R.as_dict(np.array([[0, 0, 0], [1, 0, 0]], np.int32), np.full((2, nv), 0.5, F), np.full((2, nv), 2.0, F),
                      np.full((2, nv, 4), 10, np.uint8))
    bi = np.array([[1, 0, 0], [5, 5, 5]], np.int32)
    words = R.tsdf_words(np.full((2, nv), -0.5, F), np.full((2, nv), 2.0, F), np.full((2, nv, 4), 30, np.uint8))
    up = R.deserialize(layer, R.UPDATE, bi, words)
    assert sorted(up) == [(0, 0, 0), (1, 0, 0), (5, 5, 5)] and up[(1, 0, 0)][0][0] == F(-0.5) and up[(0, 0, 0)][0][0] == F(0.5)
    assert up[(1, 0, 0)][2][0].tolist() == [30] * 4
    me = R.deserialize(layer, R.MERGE, bi, words)
    assert me[(1, 0, 0)][0][0] == 0 and me[(1, 0, 0)][1][0] == 4 and me[(1, 0, 0)][2][0].tolist() == [20] * 4
    assert me[(5, 5, 5)][0][0] == F(-0.5) and me[(5, 5, 5)][2][0].tolist() == [30] * 4       # absent: the message's voxels
    re_ = R.deserialize(layer, R.RESET, bi, words)
    assert sorted(re_) == [(1, 0, 0), (5, 5, 5)] and R.same_layers(re_, R.deserialize({}, R.UPDATE, bi, words))
    assert R.deserialize(layer, R.RESET, bi[:0], words[:0]) == {}
    assert layer[(1, 0, 0)][0][0] == F(0.5)                                                 # the input is not modified


def test_surface_bytes_by_hand():
    xyz = np.array([[1.0, -2.0, 0.5], [-0.0, 3.0, 4.0]], F)
    wgt = np.array([2.5, -0.0], F)
    b = R.surface_bytes(xyz, wgt)
    assert b.shape == (2, 32)
    assert bytes(b[0]) == struct.pack("<4f", 1.0, -2.0, 0.5, 1.0) + struct.pack("<f", 2.5) + b"\x00" * 12
    assert bytes(b[1]) == b"\x00\x00\x00\x80" + struct.pack("<3f", 3.0, 4.0, 1.0) + b"\x00\x00\x00\x80" + b"\x00" * 12
    T = np.array([[0, -1, 0, 10], [1, 0, 0, 20], [0, 0, 1, 30]], F)
    t = R.surface_bytes(xyz, wgt, T)
    assert np.frombuffer(bytes(t[0][:12]), F).tolist() == [12.0, 21.0, 30.5]
    # the association: ((m0 x + m1 y) + m2 z) + t, each in f32
    m = np.array([[0.1, 0.7, -0.3, 0.9]] * 3, F)
    p = np.array([[0.3, 0.9, 0.7]], F)
    want = F(F(F(F(m[0, 0] * p[0, 0]) + F(m[0, 1] * p[0, 1])) + F(m[0, 2] * p[0, 2])) + m[0, 3])
    assert R.transform_points(p, m)[0, 0] == want
