"""Map messages on the device (vgx_tsdf_layer_serialize, vgx_submap_serialize_layer, vgx_submap_surface_msg,
vgx_tsdf_layer_deserialize[_msg]) against the numpy restatement of tests/map_msg_ref.py, bit for bit, and every refusal.
The layers are the scenes of tests/layer_cloud_scenes.py (planted NaN and infinite distances, -0.0, weight-0 voxels, random
colours, block boxes far from the origin, vps 8 and 16), an integrated layer, its finished submap and a projected map."""
import numpy as np
import pytest

from oracle import synth
from tests import layer_cloud_scenes as S
from tests import map_msg_ref as R
from tests import scan_msg_ref as SR
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ("random_vps8", "random_vps16", "far_vps8", "far_vps16")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _layer_dict(layer):
    return R.as_dict(*layer.download())


def _assert_layer_msg(msg, kind, bi, words, what):
    k, n, wpv, nbytes = msg.stats()
    gbi, gw = msg.download()
    print(what, "blocks", n, "expected", len(bi), "bytes", nbytes)
    assert (k, n, wpv, nbytes) == (kind, len(bi), 3 if kind == capi.MSG_TSDF_LAYER else 2, words.nbytes), what
    assert R.same(gbi, np.ascontiguousarray(bi, np.int32)) and R.same(gw, words), what


def _plant(sc):
    """the scenes' own plants plus colours with four distinct bytes and every special in one known voxel run"""
    sc.rgba[0, 0] = [1, 2, 3, 4]
    sc.d[0, :5] = [np.nan, np.inf, -np.inf, -0.0, 0.25]
    sc.w[0, :5] = [1.0, 0.0, -0.0, 2.0, np.nan]
    sc.d[1, 0] = np.array([0x7fc12345], np.uint32).view(F)[0]           # a NaN payload
    return sc


@pytest.mark.parametrize("name", SCENES)
def test_serialize_every_source_bit_exact(ctx, name):
    sc = _plant(S.SCENES[name]())
    sm = capi.Submap(ctx, 0, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    layer = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
    layer.upload(sc.bi, sc.d, sc.w, sc.rgba)
    msg = capi.MapMsg(ctx)
    bi, d, w, rgba = layer.download()
    words = R.tsdf_words(d, w, rgba)
    assert R.same(bi, sc.bi) and R.same(words, R.tsdf_words(sc.d, sc.w, sc.rgba))
    _assert_layer_msg(layer.serialize(msg), capi.MSG_TSDF_LAYER, bi, words, (name, "layer"))
    assert words[0, 2] == 4 | 3 << 8 | 2 << 16 | 1 << 24 and words[1, 0] == 0x7fc12345
    assert msg.layer_geometry() == (float(F(sc.voxel_size)), sc.vps) and all(msg.device_pointers())
    td, tw, ed, eo = sm.download_layers(sc.vps)
    _assert_layer_msg(sm.serialize_layer("tsdf", msg), capi.MSG_TSDF_LAYER, sm.block_index(), R.tsdf_words(td, tw), (name, "tsdf"))
    assert R.same(td, sc.d) and R.same(tw, sc.w)
    _assert_layer_msg(sm.serialize_layer("esdf", msg), capi.MSG_ESDF_LAYER, sm.block_index(), R.esdf_words(ed, eo), (name, "esdf"))
    assert (eo == 200).any() and np.isnan(ed).any()                       # observed bytes other than 1 become the word 1
    for h in (msg, layer, sm):
        h.destroy()


def _lidar_scan():
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, 256, endpoint=False) + (2 * np.pi / 256) / 3.0, np.linspace(-0.3, 0.3, 12) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    lo, hi = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    return (d * t[:, None]).astype(F), np.random.default_rng(1).integers(0, 256, (len(d), 4), dtype=np.uint8)


@pytest.mark.parametrize("vps", [8, 16])
def test_an_integrated_layer_its_finished_submap_and_a_projected_map(ctx, vps):
    vs = 0.2
    pts, colors = _lidar_scan()
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    msg = capi.MapMsg(ctx)
    for k in range(2):
        integ.integratePointCloud(np.array([1, 0, 0, 0, 0.1 + 0.3 * k, -0.05, 0.02], F), pts, colors)
    layer.serialize(msg)                                                   # (behind the queued scans, without a stats call first)
    bi, d, w, rgba = layer.download()
    _assert_layer_msg(msg, capi.MSG_TSDF_LAYER, bi, R.tsdf_words(d, w, rgba), ("integrated", vps))
    assert len(bi) > 10 and np.unique(rgba.reshape(-1, 4), axis=0).shape[0] > 10 and (w == 0).any() and (w > 0).any()
    sm = capi.Submap.from_tsdf_layer(ctx, layer, 3)
    sm.generate_esdf()
    td, tw, ed, eo = sm.download_layers(vps)
    _assert_layer_msg(sm.serialize_layer("tsdf", msg), capi.MSG_TSDF_LAYER, sm.block_index(), R.tsdf_words(td, tw), ("finished tsdf", vps))
    _assert_layer_msg(sm.serialize_layer("esdf", msg), capi.MSG_ESDF_LAYER, sm.block_index(), R.esdf_words(ed, eo), ("finished esdf", vps))
    assert eo.any() and not eo.all()
    # the projected map of two posed copies, then its message; merging again into the same layer and serialising again
    proj = capi.TsdfLayer(ctx, vs, vps)
    poses = np.array([[1, 0, 0, 0, 0, 0, 0], [np.cos(0.2), 0, 0, np.sin(0.2), 0.37, -0.21, 0.05]], F)
    sm2 = capi.Submap.from_tsdf_layer(ctx, layer, 4)
    capi.projected_map(ctx, [sm, sm2], poses, proj)
    proj.serialize(msg)
    pbi, pd, pw, prgba = proj.download()
    _assert_layer_msg(msg, capi.MSG_TSDF_LAYER, pbi, R.tsdf_words(pd, pw, prgba), ("projected", vps))
    assert len(pbi) >= len(bi)
    for h in (msg, proj, sm2, sm, integ, layer):
        h.destroy()


def test_empty_sources_and_handle_reuse(ctx):
    msg = capi.MapMsg(ctx)
    assert msg.stats() == (capi.MSG_NONE, 0, 0, 0) and msg.device_pointers() == (None, None)
    empty = capi.TsdfLayer(ctx, 0.1, 16)
    empty.serialize(msg)
    assert msg.stats() == (capi.MSG_TSDF_LAYER, 0, 3, 0) and msg.device_pointers() == (None, None)
    assert [a.shape for a in msg.download()] == [(0, 3), (0, 3 * 4096)]
    none = capi.Submap(ctx, 1, 0.1, 8, np.zeros((0, 3), np.int32), np.zeros((0, 512), F), np.zeros((0, 512), F))
    none.serialize_layer("esdf", msg)
    assert msg.stats() == (capi.MSG_ESDF_LAYER, 0, 2, 0)
    none.set_points(capi.POINTS_VOXELS, np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, F))
    none.surface_msg(capi.POINTS_VOXELS, None, msg)
    assert msg.stats() == (capi.MSG_SURFACE_CLOUD, 0, 0, 0) and msg.download().shape == (0, 32)
    # grows, shrinks, grows: one handle through three kinds
    big, small = S.SCENES["random_vps16"](), S.SCENES["random_vps8"]()
    for sc in (big, small, big):
        layer = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
        layer.upload(sc.bi, sc.d, sc.w, sc.rgba)
        _assert_layer_msg(layer.serialize(msg), capi.MSG_TSDF_LAYER, sc.bi, R.tsdf_words(sc.d, sc.w, sc.rgba), "reuse")
        layer.destroy()
    for h in (none, empty, msg):
        h.destroy()


@pytest.mark.parametrize("name", ["far_vps8", "random_vps16"])
def test_round_trip_through_host_arrays_and_through_the_handle(ctx, name):
    sc = _plant(S.SCENES[name]())
    src = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
    src.upload(sc.bi, sc.d, sc.w, sc.rgba)
    msg = src.serialize()
    bi, words = msg.download()
    want = _layer_dict(src)
    assert len(want) == len(sc.bi)
    for form in ("host", "handle"):
        dst = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
        # something to reset: blocks the message does not hold, and one it does
        junk = np.concatenate([sc.bi[:1], sc.bi[:3] + np.int32(20)])
        dst.upload(junk, np.ones((4, sc.vps ** 3), F), np.ones((4, sc.vps ** 3), F), np.full((4, sc.vps ** 3, 4), 9, np.uint8))
        if form == "host":
            dst.deserialize(capi.MSG_ACTION_RESET, bi, words)
        else:
            dst.deserialize_msg(capi.MSG_ACTION_RESET, msg)
        got = _layer_dict(dst)
        assert R.same_layers(got, want), (name, form)
        assert dst.stats() == (len(sc.bi), 0)
        # RESET with an empty message empties the layer, and what it freed is fresh again: a scan integrated into it
        # gives what it gives in a new layer
        dst.deserialize(capi.MSG_ACTION_RESET, bi[:0], words[:0])
        assert dst.stats() == (0, 0)
        if form == "host":
            pts, colors = _lidar_scan()
            layers = []
            for target in (dst, capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)):
                integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), target)
                integ.integratePointCloud(np.array([1, 0, 0, 0, 0.1, -0.05, 0.02], F), pts, colors)
                layers.append(_layer_dict(target))
                integ.destroy()
            target.destroy()
            assert len(layers[0]) > 10 and R.same_layers(layers[0], layers[1])
            dst.deserialize(capi.MSG_ACTION_RESET, bi[:0], words[:0])
        zero = R.tsdf_words(np.zeros((1, sc.vps ** 3), F), np.zeros((1, sc.vps ** 3), F), np.zeros((1, sc.vps ** 3, 4), np.uint8))
        dst.deserialize(capi.MSG_ACTION_MERGE, junk[1:2], zero)
        dst.deserialize(capi.MSG_ACTION_MERGE, sc.bi[:1], words[:1])
        again = _layer_dict(dst)
        assert sorted(again) == sorted(tuple(int(v) for v in b) for b in (junk[1], sc.bi[0]))
        assert R.same_layers(again, R.deserialize(R.deserialize({}, R.MERGE, junk[1:2], zero), R.MERGE, sc.bi[:1], words[:1]))
        dst.destroy()
    msg.destroy()
    src.destroy()


def _merge_scene(seed, vps, box_min):
    """a layer and a message with overlapping and disjoint blocks; finite distances, weights >= 0 with zeros planted so
    that w' = 0, wA = 0 < wB and wB = 0 < wA all occur among the overlapping voxels"""
    rng = np.random.default_rng(seed)
    nv = vps ** 3
    pool = synth.dense_block_index(box_min, (4, 3, 3))
    pool = np.ascontiguousarray(pool[rng.permutation(len(pool))], np.int32)
    layer_bi, msg_bi = pool[:20], pool[12:30]                              # 8 shared, 12 + 10 on one side only

    def fill(n):
        d = rng.uniform(-0.4, 0.4, (n, nv)).astype(F)
        d[rng.random((n, nv)) < 0.02] = F(-0.0)
        w = rng.uniform(0.0, 40.0, (n, nv)).astype(F)
        w[rng.random((n, nv)) < 0.3] = F(0.0)
        w[rng.random((n, nv)) < 0.02] = F(1e-30)
        return d, w, rng.integers(0, 256, (n, nv, 4), dtype=np.uint8)
    return layer_bi, fill(len(layer_bi)), msg_bi, fill(len(msg_bi))


@pytest.mark.parametrize("vps,box_min", [(8, (-2, -1, -1)), (16, (40, -46, 43))])
@pytest.mark.parametrize("action", [R.UPDATE, R.MERGE])
def test_update_and_merge_against_the_restatement(ctx, vps, box_min, action):
    vs = 0.1
    lbi, (ld, lw, lc), mbi, (md, mw, mc) = _merge_scene(vps + action, vps, box_min)
    words = R.tsdf_words(md, mw, mc)
    start = R.as_dict(lbi, ld, lw, lc)
    want = R.deserialize(start, action, mbi, words)
    shared = [k for k in start if k in R.as_dict(mbi, md, mw, mc)]
    assert len(shared) == 8 and len(want) == 30
    if action == R.MERGE:
        a, b = R.as_dict(mbi, md, mw, mc), start
        wa = np.stack([a[k][1] for k in shared])
        wb = np.stack([b[k][1] for k in shared])
        assert ((wa + wb) == 0).sum() > 50 and ((wa == 0) & (wb > 0)).sum() > 50 and ((wb == 0) & (wa > 0)).sum() > 50
        assert any(not R.same(want[k][2], start[k][2]) for k in shared)                  # colours really blend
    runs = []
    for run in range(2):
        layer = capi.TsdfLayer(ctx, vs, vps)
        layer.upload(lbi, ld, lw, lc)
        if run == 0:
            layer.deserialize(action, mbi, words)
        else:                                                              # the handle form: a message made on the device
            src = capi.TsdfLayer(ctx, vs, vps)
            src.upload(mbi, md, mw, mc)
            msg = src.serialize()
            layer.deserialize_msg(action, msg)
            msg.destroy()
            src.destroy()
        runs.append(_layer_dict(layer))
        assert layer.stats() == (30, 0)
        layer.destroy()
    assert R.same_layers(runs[0], want), (vps, action)
    assert R.same_layers(runs[1], runs[0])


def _surface_submap(ctx):
    ref, _ = synth.config1_pair()
    sm = capi.Submap(ctx, 0, ref.voxel_size, ref.vps, ref.block_index, ref.tsdf_distance, ref.tsdf_weight, ref.esdf_distance,
                     ref.esdf_observed)
    return sm


def test_surface_cloud_bytes_and_the_scan_decoder_reads_them_back(ctx):
    sm = _surface_submap(ctx)
    n_iso, n_vox = sm.extract_isosurface_points(), sm.extract_voxel_points()
    assert n_iso > 50 and n_vox > 50 and n_iso != n_vox
    msg, scan = capi.MapMsg(ctx), capi.Scan(ctx)
    # a rotation about a tilted axis: every product is inexact in f32, a fused multiply-add would change low bits
    ax = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    T = np.concatenate([Rm, [[1.37], [-2.91], [0.63]]], 1).astype(F)
    for ptype, n in ((capi.POINTS_ISOSURFACE, n_iso), (capi.POINTS_VOXELS, n_vox)):
        xyz, _, wgt = sm.download_points(ptype)
        for t in (None, T):
            sm.surface_msg(ptype, t, msg)
            data = msg.download()
            assert msg.stats() == (capi.MSG_SURFACE_CLOUD, n, 0, 32 * n)
            assert R.same(data, R.surface_bytes(xyz, wgt, t)), (ptype, t is not None)
        # contraction would show: the transformed positions differ from the f64-accumulated ones in at least one low bit
        moved = R.transform_points(xyz, T)
        fused = (T[:, :3].astype(np.float64) @ xyz.T.astype(np.float64) + T[:, 3:].astype(np.float64)).T.astype(F)
        assert (moved.view(np.uint32) != fused.view(np.uint32)).any()
        # the existing scan decoder reads the bytes back: the submap's own points, the grey level of their weights
        sm.surface_msg(ptype, None, msg)
        _, d_payload = msg.device_pointers()
        assert scan.decode_msg_device(capi.surface_msg_layout(n), d_payload, 32 * n) == (n, 0)
        p, c = scan.download()
        assert R.same(p, xyz) and np.array_equal(c[:, 0], SR.gray(wgt, 0, 10000)) and (c[:, 3] == 255).all()
        assert scan.decode_msg(capi.surface_msg_layout(n), msg.download().tobytes()) == (n, 0) and R.same(scan.download()[0], xyz)
    # an uploaded set: weights of every kind travel bit for bit, positions with -0.0 too
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-3, 3, (1027, 3)).astype(F)
    xyz[::50, 1] = F(-0.0)
    wgt = rng.uniform(0, 12000, 1027).astype(F)
    wgt[:6] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40]
    sm.set_points(capi.POINTS_VOXELS, xyz, np.zeros(1027, F), wgt)
    for t in (None, T):
        assert R.same(sm.surface_msg(capi.POINTS_VOXELS, t, msg).download(), R.surface_bytes(xyz, wgt, t))
    for h in (scan, msg, sm):
        h.destroy()


def _refused(ctx, call, code=capi.ERR_INVALID, says=None):
    with pytest.raises(capi.VgxError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if says:
        assert says in str(e.value), str(e.value)


def test_every_refusal_leaves_its_target_unchanged(ctx):
    sc = S.SCENES["random_vps8"]()
    vps, nv = sc.vps, sc.vps ** 3
    layer = capi.TsdfLayer(ctx, sc.voxel_size, vps)
    layer.upload(sc.bi, sc.d, sc.w, sc.rgba)
    before = _layer_dict(layer)
    msg = layer.serialize()
    bi, words = msg.download()
    held = (msg.stats(), bi.copy(), words.copy())
    lib = ctx.lib
    des = lambda **kw: layer.deserialize(kw.pop("action", capi.MSG_ACTION_UPDATE), kw.pop("bi", bi), kw.pop("words", words), **kw)
    _refused(ctx, lambda: des(vps=16), says="voxels_per_side")
    _refused(ctx, lambda: des(voxel_size=sc.voxel_size * 2), says="voxel_size")
    _refused(ctx, lambda: des(voxel_size=sc.voxel_size + 3e-5), says="voxel_size")
    _refused(ctx, lambda: des(voxel_size=float("nan")), says="voxel_size")
    _refused(ctx, lambda: des(layer_type=capi.EVAL_LAYER_ESDF), says="not TSDF")
    _refused(ctx, lambda: des(words=words.reshape(-1)[:-1]), says="length")
    _refused(ctx, lambda: des(words=np.concatenate([words.reshape(-1), words.reshape(-1)[:3]])), says="length")
    _refused(ctx, lambda: des(action=3), says="unknown action")
    _refused(ctx, lambda: des(action=-1), says="unknown action")
    dup = bi.copy()
    dup[-1] = dup[2]
    _refused(ctx, lambda: des(bi=dup), says="twice")
    _refused(ctx, lambda: ctx.check(lib.vgx_tsdf_layer_deserialize(layer.h, 0, capi.EVAL_LAYER_TSDF, sc.voxel_size, vps, len(bi), None, None,
                                                                   words.size)), says="NULL arrays")
    _refused(ctx, lambda: ctx.check(lib.vgx_tsdf_layer_deserialize(layer.h, 0, capi.EVAL_LAYER_TSDF, sc.voxel_size, vps, -1, None, None, 0)),
             says="n_blocks < 0")
    assert lib.vgx_tsdf_layer_deserialize(None, 0, capi.EVAL_LAYER_TSDF, sc.voxel_size, vps, 0, None, None, 0) == capi.ERR_INVALID
    des(voxel_size=sc.voxel_size + 5e-6, bi=bi[:0], words=words[:0])          # inside the tolerance, n = 0: VGX_OK, nothing changes
    # the handle form: an ESDF message, a cloud, an empty handle, a handle of another layer geometry, another context
    sm = capi.Submap(ctx, 0, sc.voxel_size, vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    other = capi.MapMsg(ctx)
    _refused(ctx, lambda: layer.deserialize_msg(capi.MSG_ACTION_RESET, other), says="no layer message")
    sm.serialize_layer("esdf", other)
    _refused(ctx, lambda: layer.deserialize_msg(capi.MSG_ACTION_RESET, other), says="not TSDF")
    sm.set_points(capi.POINTS_VOXELS, np.ones((5, 3), F), np.ones(5, F), np.ones(5, F))
    sm.surface_msg(capi.POINTS_VOXELS, None, other)
    _refused(ctx, lambda: layer.deserialize_msg(capi.MSG_ACTION_RESET, other), says="no layer message")
    l16 = capi.TsdfLayer(ctx, sc.voxel_size, 16)
    _refused(ctx, lambda: l16.deserialize_msg(capi.MSG_ACTION_RESET, msg), says="voxels_per_side")
    _refused(ctx, lambda: layer.deserialize_msg(7, msg), says="unknown action")
    _refused(ctx, lambda: ctx.check(lib.vgx_tsdf_layer_deserialize_msg(layer.h, 0, None)), says="NULL message")
    assert R.same_layers(_layer_dict(layer), before) and l16.stats() == (0, 0)
    # producers: the handle keeps what it held
    sm.surface_msg(capi.POINTS_VOXELS, None, other)
    kept = (other.stats(), other.download().copy())
    _refused(ctx, lambda: sm.surface_msg(2, None, other), says="point type")
    _refused(ctx, lambda: sm.surface_msg(-1, None, other), says="point type")
    _refused(ctx, lambda: sm.surface_msg(capi.POINTS_ISOSURFACE, None, other), says="never extracted")
    for bad in (np.nan, np.inf, -np.inf):
        T = np.eye(4, dtype=F)[:3].copy()
        T[1, 2] = bad
        _refused(ctx, lambda: sm.surface_msg(capi.POINTS_VOXELS, T, other), says="not finite")
    _refused(ctx, lambda: sm.serialize_layer(2, other), says="neither")
    _refused(ctx, lambda: ctx.check(lib.vgx_submap_serialize_layer(None, 1, other.h)), says="NULL submap")
    _refused(ctx, lambda: ctx.check(lib.vgx_submap_surface_msg(None, 0, None, other.h)), says="NULL submap")
    _refused(ctx, lambda: ctx.check(lib.vgx_tsdf_layer_serialize(None, other.h)), says="NULL layer")
    _refused(ctx, lambda: ctx.check(lib.vgx_tsdf_layer_serialize(layer.h, None)), says="NULL message")
    _refused(ctx, lambda: ctx.check(lib.vgx_submap_serialize_layer(sm.h, 1, None)), says="NULL message")
    tsdf_only = capi.Submap(ctx, 2, sc.voxel_size, vps, sc.bi, sc.d, sc.w)
    _refused(ctx, lambda: tsdf_only.serialize_layer("esdf", other), says="not resident")
    tsdf_only.serialize_layer("tsdf", msg)
    tsdf_only.release_raw_layers()
    _refused(ctx, lambda: tsdf_only.serialize_layer("tsdf", other), says="not resident")
    assert other.stats() == kept[0] and R.same(other.download(), kept[1])
    _assert_layer_msg(msg, capi.MSG_TSDF_LAYER, sc.bi, R.tsdf_words(sc.d, sc.w), "kept")
    _refused(ctx, lambda: ctx.check(lib.vgx_map_msg_download(other.h, bi.ctypes.data_as(capi.i32p), None)), says="no block indices")
    _refused(ctx, lambda: other.layer_geometry(), says="no layer message")
    ctx2 = capi.Context(0)
    foreign = capi.MapMsg(ctx2)
    _refused(ctx, lambda: layer.serialize(foreign), says="another context")
    _refused(ctx, lambda: sm.serialize_layer("tsdf", foreign), says="another context")
    _refused(ctx, lambda: sm.surface_msg(capi.POINTS_VOXELS, None, foreign), says="another context")
    _refused(ctx, lambda: layer.deserialize_msg(0, foreign), says="another context")
    assert foreign.stats() == (capi.MSG_NONE, 0, 0, 0)
    foreign.destroy()
    ctx2.close()
    assert R.same_layers(_layer_dict(layer), before)
    assert held[0] == (capi.MSG_TSDF_LAYER, len(bi), 3, words.nbytes)
    for h in (tsdf_only, l16, other, sm, msg, layer):
        h.destroy()


def test_seeded_fuzz_of_serialise_and_the_three_actions(ctx):
    """a few dozen small random layers and messages (profiles/fuzz_map_layers.py's style): serialise, then every action"""
    rng = np.random.default_rng(20261017)
    msg = capi.MapMsg(ctx)
    for case in range(36):
        vps = (8, 16)[case % 2]
        nv = vps ** 3
        vs = float(rng.choice([0.05, 0.1, 0.2]))
        origin = rng.integers(-60, 60, 3)
        pool = np.ascontiguousarray(synth.dense_block_index(tuple(int(v) for v in origin), (3, 3, 2))[rng.permutation(18)], np.int32)
        nl, nm, shift = int(rng.integers(0, 10)), int(rng.integers(0, 10)), int(rng.integers(0, 9))

        def fill(n):
            d = rng.uniform(-0.5, 0.5, (n, nv)).astype(F)
            w = np.where(rng.random((n, nv)) < 0.4, F(0), rng.uniform(0, 100, (n, nv)).astype(F)).astype(F)
            return d, w, rng.integers(0, 256, (n, nv, 4), dtype=np.uint8)
        lbi, mbi = pool[:nl], pool[shift:shift + nm]
        (ld, lw, lc), (md, mw, mc) = fill(len(lbi)), fill(len(mbi))
        src = capi.TsdfLayer(ctx, vs, vps)
        src.upload(mbi, md, mw, mc)
        words = R.tsdf_words(md, mw, mc)
        _assert_layer_msg(src.serialize(msg), capi.MSG_TSDF_LAYER, mbi, words, ("fuzz", case))
        for action in (R.UPDATE, R.MERGE, R.RESET):
            layer = capi.TsdfLayer(ctx, vs, vps)
            layer.upload(lbi, ld, lw, lc)
            if (case + action) % 2:
                layer.deserialize_msg(action, msg)
            else:
                layer.deserialize(action, mbi, words)
            want = R.deserialize(R.as_dict(lbi, ld, lw, lc), action, mbi, words)
            assert R.same_layers(_layer_dict(layer), want), (case, action)
            layer.destroy()
        src.destroy()
    msg.destroy()
