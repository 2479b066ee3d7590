"""The elevation map on the device (vgx_tsdf_layer_elevation_map, vgx_submap_layer_elevation_map) against the numpy
restatement of tests/elevation_map_ref.py byte for byte -- box, the eleven arrays, both totals -- and every refusal.  The
scenes are those of tests/elevation_map_scenes.py (checked on the CPU not to pass on nothing)."""
import ctypes as C

import numpy as np
import pytest

from tests import elevation_map_ref as R
from tests import elevation_map_scenes as S
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _assert_map(em, want, what):
    (x0, y0), (w, h), vs, states, classes = em.stats()
    print(what, "box", (x0, y0, w, h), "expected", (want.x0, want.y0, want.W, want.H), "states", states, "expected", want.state_counts,
          "classes", classes, "expected", want.class_counts)
    assert (w, h) == (want.W, want.H), what
    if w * h > 0 or want.W + want.H > 0:
        assert (x0, y0) == (want.x0, want.y0), what
    assert states == want.state_counts and classes == want.class_counts, what
    got = em.download()
    for name, a in zip(R.FIELDS, got):
        b = getattr(want, name)
        assert a.dtype == b.dtype and R.same(a, b), (what, name, int((R.bits(a) != R.bits(b)).sum()))
    return got


def _sources(ctx, sc):
    sm = capi.Submap(ctx, 0, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    layer = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
    layer.upload(sc.bi, sc.d, sc.w)
    return sm, layer


def _run(source, sm, layer, cfg, em):
    if source == "layer":
        return layer.elevation_map(capi.elevation_map_config(**cfg), em)
    return sm.layer_elevation_map(source, capi.elevation_map_config(**cfg), em)


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_maps_byte_exact_in_every_source_kind_and_configuration(ctx, name):
    sc = S.SCENES[name]()
    sm, layer = _sources(ctx, sc)
    em = capi.ElevationMap(ctx)
    for cfg in sc.configs:
        for source in S.SOURCES:
            _assert_map(_run(source, sm, layer, cfg, em), S.reference(sc, cfg, source), (name, source, cfg))
    for h in (em, layer, sm):
        h.destroy()


def _device_read(ptr, like):
    out = np.empty_like(like)
    hip = C.CDLL(None)          # the HIP runtime the library itself runs on (capi.load opens it globally)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0    # device to host
    return out


def test_handle_reuse_device_pointers_and_run_to_run_identity(ctx):
    """one handle through maps that shrink, vanish and grow again; the device pointers are the download; a second handle
    and a second run give the same bytes"""
    sc = S.SCENES["box_vps8"]()
    sm, layer = _sources(ctx, sc)
    em, other = capi.ElevationMap(ctx), capi.ElevationMap(ctx)
    assert em.stats() == ((0, 0), (0, 0), 0.0, (0, 0, 0, 0), (0, 0, 0)) and em.device_pointers() == (None,) * 11
    assert [a.shape for a in em.download()] == [(0, 0, 2) if n == "grad" else (0, 0) for n in R.FIELDS]
    band = {k: sc.configs[0][k] for k in ("z_min", "z_max", "max_distance_m", "step_radius_cells")}
    order = [dict(band), dict(band, use_box=1, cell_min=(-3, -2), cell_dim=(5, 4)), dict(band, use_box=1, cell_min=(0, 0), cell_dim=(0, 0)),
             dict(band, z_min=50.0, z_max=51.0), dict(band, use_box=1, cell_min=(-30, -20), cell_dim=(63, 50)), dict(band)]
    for k, cfg in enumerate(order):
        for source in S.SOURCES:
            want = S.reference(sc, cfg, source)
            got = _assert_map(_run(source, sm, layer, cfg, em), want, ("reuse", k, source))
            ptrs = em.device_pointers()
            if want.W * want.H == 0:
                assert ptrs == (None,) * 11
                continue
            assert all(ptrs)
            for a, p in zip(got, ptrs):
                assert R.same(_device_read(p, a), a)
            again = _run(source, sm, layer, cfg, other).download()
            assert all(R.same(a, b) for a, b in zip(got, again)) and other.stats() == em.stats()
            assert all(R.same(a, b) for a, b in zip(got, _run(source, sm, layer, cfg, em).download()))
    # the pass times are a measuring aid, off by default: zeros until asked for, and asking changes no byte
    assert em.pass_ms() == (0.0,) * 6
    em.set_timing(True)
    timed = _run("esdf", sm, layer, order[0], em).download()
    ms = em.pass_ms()
    assert all(v > 0 for v in ms) and all(R.same(a, b) for a, b in zip(timed, _run("esdf", sm, layer, order[0], other).download()))
    _run("esdf", sm, layer, order[1], em)
    assert em.pass_ms()[0] == 0.0 and all(v > 0 for v in em.pass_ms()[1:])             # a given box: no box pass
    em.set_timing(False)
    assert em.pass_ms() == (0.0,) * 6
    for h in (other, em, layer, sm):
        h.destroy()


def test_empty_sources(ctx):
    em = capi.ElevationMap(ctx)
    cfg = dict(z_min=0.0, z_max=1.0)
    box = dict(cfg, use_box=1, cell_min=(-2, 3), cell_dim=(5, 4), max_distance_m=0.3)
    empty = capi.TsdfLayer(ctx, 0.1, 16)
    none = capi.Submap(ctx, 1, 0.1, 16, np.zeros((0, 3), np.int32), np.zeros((0, 4096), F), np.zeros((0, 4096), F))
    for run in (lambda c: empty.elevation_map(capi.elevation_map_config(**c), em),
                lambda c: none.layer_elevation_map("tsdf", capi.elevation_map_config(**c), em)):
        run(cfg)
        assert em.stats()[1] == (0, 0) and em.stats()[3] == (0, 0, 0, 0) and em.stats()[4] == (0, 0, 0)
        run(box)
        assert em.stats() == ((-2, 3), (5, 4), F(0.1), (20, 0, 0, 0), (20, 0, 0))
        got = dict(zip(R.FIELDS, em.download()))
        assert all(not R.bits(got[n]).any() for n in R.FIELDS[:-1]) and (got["distance"] == F(0.3)).all()
        run(dict(box, unknown_is_obstacle=1))
        assert not R.bits(em.download()[-1]).any()
    for h in (none, empty, em):
        h.destroy()


def _lidar_scan():
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, 256, endpoint=False) + (2 * np.pi / 256) / 3.0,
                         np.linspace(-0.5, 0.3, 16) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    lo, hi = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    return (d * t[:, None]).astype(F)


@pytest.mark.parametrize("vps", [8, 16])
def test_an_integrated_layer_without_an_intervening_synchronisation(ctx, vps):
    """a room integrated scan by scan (reproducible mode), the call queued straight behind the last scan; then the
    submap finished from the layer, both of its layers"""
    vs = 0.2
    pts = _lidar_scan()
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    cfgs = (dict(z_min=-1.6, z_max=0.9, max_distance_m=1.5, max_step_m=0.3),
            dict(z_min=-1.6, z_max=0.9, max_distance_m=1.5, unknown_is_obstacle=1, step_radius_cells=3, pick=1),
            dict(z_min=-1.3, z_max=0.1, use_box=1, cell_min=(-9, -7), cell_dim=(37, 21), hole_is_obstacle=0))
    em = capi.ElevationMap(ctx)
    for k in range(3):
        integ.integratePointCloud(np.array([1, 0, 0, 0, 0.1 + 0.3 * k, -0.05, 0.02], F), pts, count=False)
    layer.elevation_map(capi.elevation_map_config(**cfgs[0]), em)                # no synchronisation in between
    bi, d, w, _ = layer.download()
    want = R.elevation_map(vs, vps, bi, d, w, False, **cfgs[0])
    _assert_map(em, want, ("integrated", vps, 0))
    with np.errstate(invalid="ignore"):
        assert want.state_counts[1] > 100 and want.state_counts[0] > 0 and ((want.t > 0) & (want.t < 1)).any()
    for cfg in cfgs[1:]:
        _assert_map(layer.elevation_map(capi.elevation_map_config(**cfg), em), R.elevation_map(vs, vps, bi, d, w, False, **cfg),
                    ("integrated", vps, cfg))
    sm = capi.Submap.from_tsdf_layer(ctx, layer, 3)
    sm.generate_esdf()
    td, tw, ed, eo = sm.download_layers(vps)
    sbi = sm.block_index()
    for source, seen, dist in (("tsdf", tw, td), ("esdf", eo, ed)):
        for cfg in cfgs:
            want = R.elevation_map(vs, vps, sbi, dist, seen, source == "esdf", **cfg)
            _assert_map(sm.layer_elevation_map(source, capi.elevation_map_config(**cfg), em), want, ("finished", vps, source, cfg))
    for h in (sm, em, integ, layer):
        h.destroy()


def test_fuzz_64_draws(ctx):
    rng = np.random.default_rng(2025)
    em = capi.ElevationMap(ctx)
    states, classes = np.zeros(4, np.int64), np.zeros(3, np.int64)
    for k in range(64):
        sc, source = S.fuzz_draw(rng)
        cfg = sc.configs[0]
        if source == "layer":
            src = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
            src.upload(sc.bi, sc.d, sc.w)
            src.elevation_map(capi.elevation_map_config(**cfg), em)
        else:
            src = capi.Submap(ctx, k, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
            src.layer_elevation_map(source, capi.elevation_map_config(**cfg), em)
        want = S.reference(sc, cfg, source)
        _assert_map(em, want, ("fuzz", k, source, cfg))
        states += want.state_counts
        classes += want.class_counts
        src.destroy()
    print("fuzz totals: states", states, "classes", classes)
    assert (states > 500).all() and (classes > 500).all(), (states, classes)
    em.destroy()


def test_refusals_leave_the_map_untouched(ctx):
    sc = S.SCENES["box_vps8"]()
    sm, layer = _sources(ctx, sc)
    tsdf_only = capi.Submap(ctx, 5, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w)          # an ESDF never generated
    released = capi.Submap(ctx, 6, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    released.release_raw_layers()
    far = capi.TsdfLayer(ctx, sc.voxel_size, 8, lut_min=(2 ** 28 - 2, 0, 0), lut_dim=(4, 2, 2), max_blocks=8)   # ix would pass 2^31
    # two blocks 2048 apart on x and y: their extent in whole blocks is 16392 x 16392 cells, more than 2^28
    wide_bi = np.array([[0, 0, 0], [2048, 2048, 0]], np.int32)
    wide_d = np.repeat(((np.arange(512) // 64 - 3.5) * sc.voxel_size).astype(F)[None], 2, 0)   # a floor between rows 3 and 4
    wide = capi.Submap(ctx, 8, sc.voxel_size, 8, wide_bi, wide_d, np.ones((2, 512), F))
    ctx2 = capi.Context(0)
    foreign = capi.ElevationMap(ctx2)
    em = capi.ElevationMap(ctx)
    good = dict(sc.configs[1])                                                   # a box larger than the layer: every state and class
    sm.layer_elevation_map("esdf", capi.elevation_map_config(**good), em)
    held, held_stats = em.download(), em.stats()
    assert held[0].size > 0 and min(held_stats[3]) > 0 and min(held_stats[4]) > 0
    lib = ctx.lib

    def cfgp(**kw):
        return C.byref(capi.elevation_map_config(**dict(good, **kw)))

    bad_cfgs = [dict(z_min=np.nan), dict(z_max=np.nan), dict(z_min=-np.inf), dict(z_max=np.inf), dict(z_min=1.0, z_max=0.5),
                dict(min_weight=-1e-3), dict(min_weight=np.nan), dict(min_weight=np.inf), dict(min_free_voxels=0),
                dict(min_free_voxels=-2), dict(max_distance_m=0.0), dict(max_distance_m=-1.0), dict(max_distance_m=np.nan),
                dict(max_distance_m=np.inf), dict(max_distance_m=2048.5 * sc.voxel_size),                              # R = 2049
                dict(pick=2), dict(pick=-1), dict(step_radius_cells=-1), dict(step_radius_cells=65), dict(min_support=0),
                dict(min_support=-3), dict(min_headroom_voxels=0), dict(min_headroom_voxels=-1), dict(max_slope=np.nan),
                dict(max_slope=-0.5), dict(max_slope=-np.inf), dict(max_step_m=np.nan), dict(max_step_m=-0.01),
                dict(use_box=1, cell_dim=(-1, 4)), dict(use_box=1, cell_dim=(4, -1)),
                dict(use_box=1, cell_dim=(1 << 15, (1 << 13) + 1)),                       # 2^28 + 2^15 cells
                dict(use_box=1, cell_min=(2 ** 31 - 4, 0), cell_dim=(5, 5))]               # cell_min + cell_dim overflows
    calls = []
    for kw in bad_cfgs:
        calls.append((str(kw) + " submap", lambda kw=kw: lib.vgx_submap_layer_elevation_map(sm.h, 0, cfgp(**kw), em.h)))
        calls.append((str(kw) + " layer", lambda kw=kw: lib.vgx_tsdf_layer_elevation_map(layer.h, cfgp(**kw), em.h)))
    default_only = capi.ElevationMapConfig()
    lib.vgx_elevation_map_config_default(C.byref(default_only))                            # the band never set
    calls += [
        ("defaults alone submap", lambda: lib.vgx_submap_layer_elevation_map(sm.h, 0, C.byref(default_only), em.h)),
        ("defaults alone layer", lambda: lib.vgx_tsdf_layer_elevation_map(layer.h, C.byref(default_only), em.h)),
        ("NULL cfg submap", lambda: lib.vgx_submap_layer_elevation_map(sm.h, 0, None, em.h)),
        ("NULL cfg layer", lambda: lib.vgx_tsdf_layer_elevation_map(layer.h, None, em.h)),
        ("NULL submap", lambda: lib.vgx_submap_layer_elevation_map(None, 0, cfgp(), em.h)),
        ("NULL layer", lambda: lib.vgx_tsdf_layer_elevation_map(None, cfgp(), em.h)),
        ("layer value", lambda: lib.vgx_submap_layer_elevation_map(sm.h, 2, cfgp(), em.h)),
        ("layer value -1", lambda: lib.vgx_submap_layer_elevation_map(sm.h, -1, cfgp(), em.h)),
        ("ESDF never generated", lambda: lib.vgx_submap_layer_elevation_map(tsdf_only.h, 0, cfgp(), em.h)),
        ("released ESDF", lambda: lib.vgx_submap_layer_elevation_map(released.h, 0, cfgp(), em.h)),
        ("released TSDF", lambda: lib.vgx_submap_layer_elevation_map(released.h, 1, cfgp(), em.h)),
        ("the default box beyond 2^28 cells", lambda: lib.vgx_submap_layer_elevation_map(wide.h, 1, cfgp(z_min=0.0, z_max=0.8, use_box=0), em.h)),
        ("block indices overflow", lambda: lib.vgx_tsdf_layer_elevation_map(far.h, cfgp(), em.h)),
    ]
    for what, call in calls:
        assert call() == capi.ERR_INVALID, what
        assert lib.vgx_last_error(ctx.h), what
        assert em.stats() == held_stats, what
        assert all(R.same(a, b) for a, b in zip(em.download(), held)), what
    assert b"overflow" in lib.vgx_last_error(ctx.h)
    for call in (lambda: lib.vgx_submap_layer_elevation_map(sm.h, 0, cfgp(), None), lambda: lib.vgx_tsdf_layer_elevation_map(layer.h, cfgp(), None)):
        assert call() == capi.ERR_INVALID
    # a map of another context: refused, and that map stays empty
    for call in (lambda: lib.vgx_submap_layer_elevation_map(sm.h, 0, cfgp(), foreign.h),
                 lambda: lib.vgx_tsdf_layer_elevation_map(layer.h, cfgp(), foreign.h)):
        assert call() == capi.ERR_INVALID
        assert foreign.stats()[1] == (0, 0)
    assert b"another context" in lib.vgx_last_error(ctx.h)
    assert lib.vgx_elevation_map_create(ctx.h, None) == capi.ERR_INVALID and lib.vgx_elevation_map_destroy(None) == capi.ERR_INVALID
    assert lib.vgx_elevation_map_stats(None, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.vgx_elevation_map_download(None, *([None] * 11)) == capi.ERR_INVALID
    assert lib.vgx_elevation_map_device_pointers(None, *([None] * 11)) == capi.ERR_INVALID
    assert lib.vgx_elevation_map_set_timing(None, 1) == capi.ERR_INVALID and lib.vgx_elevation_map_pass_ms(em.h, None) == capi.ERR_INVALID
    # voxels_per_side other than 8 or 16 (VGX_ERR_UNSUPPORTED in the producing calls) cannot reach them: neither source
    # kind can be created with one, so that refusal is the sources' own
    h = C.c_void_p()
    z4 = np.zeros((1, 64), F)
    assert lib.vgx_tsdf_layer_create(ctx.h, C.c_float(0.1), 4, None, None, 0, C.byref(h)) == capi.ERR_UNSUPPORTED and not h.value
    assert lib.vgx_submap_create(ctx.h, 9, C.c_float(0.1), 4, 1, wide_bi.ctypes.data_as(capi.i32p), z4.ctypes.data_as(capi.f32p),
                                 z4.ctypes.data_as(capi.f32p), None, None, C.byref(h)) == capi.ERR_UNSUPPORTED and not h.value
    # the same two blocks inside a given box are served: only the default box was too large
    small = dict(good, z_min=0.0, z_max=0.8, use_box=1, cell_min=(-2, -2), cell_dim=(12, 12))
    _assert_map(wide.layer_elevation_map("tsdf", capi.elevation_map_config(**small), em),
                R.elevation_map(sc.voxel_size, 8, wide_bi, wide_d, np.ones((2, 512), F), False, **small), "wide, boxed")
    # the limits themselves are served: R = 2048, the window 0 and 64, zero and infinite limits, and the TSDF layer of the
    # submap without an ESDF
    for edge in (dict(good, max_distance_m=2048 * sc.voxel_size), dict(good, step_radius_cells=64, max_slope=0.0, max_step_m=np.inf),
                 dict(good, step_radius_cells=0, max_slope=np.inf, max_step_m=0.0)):
        _assert_map(tsdf_only.layer_elevation_map("tsdf", capi.elevation_map_config(**edge), em), S.reference(sc, edge, "tsdf"),
                    ("after the refusals", edge))
    foreign.destroy()
    ctx2.close()
    for h in (em, wide, far, released, tsdf_only, layer, sm):
        h.destroy()
