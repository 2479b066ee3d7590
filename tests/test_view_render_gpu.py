"""View rendering on the device (vgx_view, vgx_tsdf_layer_render_view, vgx_submap_render_view) against the restatement of
tests/view_render_ref.py, bit for bit on every output array and count: a random uploaded layer (holes, zero weights,
shuffled slots, vps 8 and 16; a full 6-DoF pose; non-finite and zero directions strewn in) at every size and image shape,
with both ray mappings and every flag; the layer the reproducible integrator built, rendered right behind an asynchronous
scan; the submap entry; colours; the points handed on by device pointer to scan registration and to an integrator; and
every refusal."""
import math
import types

import numpy as np
import pytest

from tests import scan_registration_ref as R
from tests import view_render_ref as V
from tests.test_map_query_gpu import _full_pose, _random_submap
from voxgraph_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
SHAPES = [(1, 1), (7, 3), (8, 8), (9, 9), (37, 5), (64, 16)]            # (width, height)
FLAGS = [capi.VIEW_POINTS, capi.VIEW_GRADIENT, capi.VIEW_WEIGHT, capi.VIEW_RGBA, capi.VIEW_N_SAMPLES]
# the random layers have 0.1 m voxels: a quarter voxel, a voxel, three voxels
CFG = dict(s_max=6.0, min_step=0.025, unknown_step=0.1, max_bracket=0.3)
ROOM_CFG = dict(s_max=12.0, min_step=0.05, unknown_step=0.2, max_bracket=0.65)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _scene(vps):
    """(submap data with colours, pose, 1024 directions): needs no device, so that the restatement can be looked at alone"""
    rng = np.random.default_rng(70 + vps)
    d = _random_submap(rng, vps)
    d.tsdf_rgba = rng.integers(0, 256, d.tsdf_distance.shape + (4,), dtype=np.uint8)
    T = _full_pose(rng)
    dirs = rng.normal(size=(1024, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs[::7] *= rng.uniform(0.3, 3.0, (len(dirs[::7]), 1))             # the library never normalises
    dirs = dirs.astype(F)
    bad = rng.random(len(dirs)) < 0.04
    dirs[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum())).astype(F)
    dirs[rng.random(len(dirs)) < 0.02] = rng.choice([0.0, -0.0], 3).astype(F)
    return d, T, dirs


def _ref_layer(d, colours=True):
    return V.layer_of(d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.tsdf_rgba if colours else None)


def _same(view, want, flags=capi.VIEW_ALL):
    got = view.download()
    assert view.stats() == want.counts, (view.stats(), want.counts)
    held = dict(points=capi.VIEW_POINTS, gradient=capi.VIEW_GRADIENT, weight=capi.VIEW_WEIGHT, rgba=capi.VIEW_RGBA,
                n_samples=capi.VIEW_N_SAMPLES)
    for name in capi.ViewImage._fields:
        g = getattr(got, name)
        if name in held and not flags & held[name]:
            assert g is None
            continue
        assert np.array_equal(_bits(g), _bits(getattr(want, name))), (name, int((g != getattr(want, name)).sum()))
    return got


@pytest.fixture(scope="module", params=[8, 16])
def random_scene(request, ctx):
    vps = request.param
    d, T, dirs = _scene(vps)
    layer = capi.TsdfLayer(ctx, d.voxel_size, vps)
    layer.upload(d.block_index, d.tsdf_distance, d.tsdf_weight, d.tsdf_rgba)
    yield layer, _ref_layer(d), T, dirs, d
    layer.destroy()


def test_random_layer_at_every_size(ctx, random_scene):
    layer, L, T, dirs, _ = random_scene
    view = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **CFG))
    for n in SIZES:
        want = V.render(L, T, dirs[:n], V.config(**CFG))
        got = _same(layer.render_view(view, T, dirs[:n]), want)
        assert len(got.range) == n
    # the largest case holds every status, rays of many lengths, and colours
    assert sorted(np.unique(got.status)) == [capi.VIEW_MISS, capi.VIEW_HIT, capi.VIEW_INSIDE, capi.VIEW_BAD, capi.VIEW_HIT_UNSAMPLED]
    assert got.n_samples.max() > 8 * max(got.n_samples[got.status == capi.VIEW_HIT].min(), 1) and got.rgba.any()
    # the handle is reused: a smaller view after a larger one holds the smaller one alone
    _same(layer.render_view(view, T, dirs[:65]), V.render(L, T, dirs[:65], V.config(**CFG)))
    view.destroy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_shapes_with_both_ray_mappings(ctx, random_scene, shape):
    layer, L, T, dirs, _ = random_scene
    width, height = shape
    n = width * height
    want = V.render(L, T, dirs[:n], V.config(**CFG))
    tiled = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, image_width=width, **CFG))
    linear = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **CFG))
    a = _same(layer.render_view(tiled, T, dirs[:n]), want)
    b = _same(layer.render_view(linear, T, dirs[:n]), want)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    if n > 1:                       # a last row that is not full: n need not be a multiple of the width
        _same(layer.render_view(tiled, T, dirs[:n - 1]), V.render(L, T, dirs[:n - 1], V.config(**CFG)))
    tiled.destroy()
    linear.destroy()


def test_each_flag_alone_and_none(ctx, random_scene):
    layer, L, T, dirs, _ = random_scene
    n = 300
    want = V.render(L, T, dirs[:n], V.config(**CFG))
    for flags in FLAGS + [0]:
        view = capi.View(ctx, capi.view_config(flags=flags, **CFG))
        _same(layer.render_view(view, T, dirs[:n]), want, flags)
        ptr = view.device_pointers()
        assert ptr.range and ptr.status
        for name, bit in zip(capi.ViewImage._fields[2:], FLAGS):
            assert bool(getattr(ptr, name)) == bool(flags & bit)
        # an output the view does not hold cannot be asked for
        if not flags & capi.VIEW_WEIGHT:
            w = np.full(n, 7.0, F)
            assert ctx.lib.vgx_view_download(view.h, None, None, None, None, capi._ptr(w, capi.f32p), None, None) == capi.ERR_INVALID
            assert (w == 7.0).all()
        view.destroy()


def test_other_configurations(ctx, random_scene):
    """a start away from the sensor, a coarse and a fine march, a narrow bracket, a short reach"""
    layer, L, T, dirs, _ = random_scene
    n = 400
    seen = set()
    for kw in (dict(s_min=0.35), dict(step_scale=1.5, min_step=0.1), dict(step_scale=0.3, min_step=0.01, unknown_step=0.03),
               dict(max_bracket=0.02), dict(s_max=0.5), dict(s_min=6.0)):
        cfg = dict(CFG, **kw)
        view = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **cfg))
        got = _same(layer.render_view(view, T, dirs[:n]), V.render(L, T, dirs[:n], V.config(**cfg)))
        seen.add(tuple(np.bincount(got.status, minlength=5)))
        view.destroy()
    assert len(seen) == 6                                   # every configuration changed the outcome


def _integrated_layer(ctx, n_scans):
    layer = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS)
    integrator = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for k in range(n_scans):
        integrator.integratePointCloud(R.pose7(R.scan_pose(k)), R.room_scan(R.scan_pose(k)))
    return layer, integrator


@pytest.fixture(scope="module")
def room_view():
    """the restatement on the CPU oracle's six-scan layer, from the seventh scan's pose: computed once"""
    raw = R.room_layer()
    L = V.layer_of(R.VOXEL_SIZE, R.VPS, raw.bi, raw.d, raw.w)
    T, dirs = R.pose7(R.scan_pose(6)), V.room_dirs()
    return T, dirs, V.render(L, T, dirs, V.config(**ROOM_CFG))


def test_render_is_ordered_behind_an_asynchronous_scan(ctx, room_view):
    """a view rendered right after vgx_tsdf_integrate(n_updates = NULL), with no synchronisation in between, sees that
    scan: the restatement's bits on the six-scan layer"""
    T, dirs, want = room_view
    layer, integrator = _integrated_layer(ctx, 5)
    view = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, image_width=256, **ROOM_CFG))
    integrator.integratePointCloud(R.pose7(R.scan_pose(5)), R.room_scan(R.scan_pose(5)), count=False)
    got = _same(layer.render_view(view, T, dirs), want)
    assert (got.status == capi.VIEW_HIT).mean() > 0.7 and not got.rgba.any()      # (the scans carried no colours)
    for x in (view, integrator, layer):
        x.destroy()


def test_submap_entry_renders_the_same_bytes(ctx, random_scene):
    import torch
    layer, L, T, dirs, d = random_scene
    n = 777
    want = V.render(L, T, dirs[:n], V.config(**CFG))
    sm = capi.Submap(ctx, 3, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.esdf_distance, d.esdf_observed)
    sm.set_colors(d.tsdf_rgba)
    a = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **CFG))
    b = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, image_width=37, **CFG))
    from_layer = _same(layer.render_view(a, T, dirs[:n]), want)
    from_submap = _same(sm.render_view(b, T, dirs[:n]), want)
    for x, y in zip(from_layer, from_submap):
        assert np.array_equal(_bits(x), _bits(y))
    # directions on the device: a torch tensor, a raw address
    dev = torch.from_numpy(dirs[:n]).cuda()
    torch.cuda.synchronize()
    _same(sm.render_view(b, T, dev), want)
    _same(layer.render_view(a, T, dev), want)
    _same(sm.render_view(b, T, dev.data_ptr(), n), want)
    _same(layer.render_view(a, T, dev.data_ptr(), n), want)
    # a submap without colours renders rgba 0; one whose raw layers were released is refused, the view left as it was
    plain = capi.Submap(ctx, 4, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.esdf_distance, d.esdf_observed)
    _same(plain.render_view(b, T, dirs[:n]), V.render(_ref_layer(d, colours=False), T, dirs[:n], V.config(**CFG)))
    before = b.download()
    plain.release_raw_layers()
    with pytest.raises(capi.VgxError) as e:
        plain.render_view(b, T, dirs[:n])
    assert e.value.code == capi.ERR_INVALID and "released" in str(e.value)
    for x, y in zip(before, b.download()):
        assert np.array_equal(_bits(x), _bits(y))
    for x in (a, b, sm, plain):
        x.destroy()


def test_colours_of_a_coloured_layer(ctx, random_scene):
    layer, L, T, dirs, d = random_scene
    view = capi.View(ctx, capi.view_config(flags=capi.VIEW_RGBA, **CFG))
    n = 1000
    want = V.render(L, T, dirs[:n], V.config(**CFG))
    got = _same(layer.render_view(view, T, dirs[:n]), want, capi.VIEW_RGBA)
    hit = got.status == capi.VIEW_HIT
    assert hit.sum() > 100 and got.rgba[hit].any(1).all() and not got.rgba[~hit].any()
    assert len(np.unique(got.rgba[hit], axis=0)) > 0.9 * hit.sum()
    view.destroy()


def test_points_compose_with_scan_registration_and_integration(ctx, room_view):
    """the view's points by device pointer into ScanRegistration.evaluate and a second layer's integrate_device: what the
    host-array paths give from the downloaded points"""
    T, dirs, want = room_view
    layer, integrator = _integrated_layer(ctx, 6)
    view = capi.View(ctx, capi.view_config(**ROOM_CFG))                  # (the default flags: points)
    got = _same(layer.render_view(view, T, dirs), want, capi.VIEW_POINTS)
    n, d_points = len(dirs), view.device_pointers().points
    n_hit = int(((got.status == capi.VIEW_HIT) | (got.status == capi.VIEW_HIT_UNSAMPLED)).sum())
    assert d_points and 0 < n_hit < n
    # rays without a hit are zero points: min_range_m > 0 drops them
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE, min_range_m=0.05))
    prior = R.pose7(R.seeded_prior(3))
    reg.set_points(d_points, n)
    by_pointer = reg.evaluate(layer, prior)
    reg.set_points(got.points)
    by_array = reg.evaluate(layer, prior)
    assert by_pointer[1:] == by_array[1:] and by_pointer[2] == n_hit and np.array_equal(_bits(by_pointer[0]), _bits(by_array[0]))
    assert by_pointer[1] > 0.5 * n_hit
    # ... and the integrators drop them while min_ray_length_m > 0
    layers = []
    for device in (True, False):
        second = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS)
        integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), second)
        updates = integ.integrate_device(T, d_points, None, n, count=True) if device else integ.integratePointCloud(T, got.points)
        layers.append((updates, second.download()))
        integ.destroy()
        second.destroy()
    (ua, a), (ub, b) = layers
    assert ua == ub > 0 and len(a[0]) > 0 and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    for x in (reg, view, integrator, layer):
        x.destroy()


def test_refusals(ctx, random_scene):
    layer, L, T, dirs, d = random_scene
    lib = ctx.lib
    f32p = capi.f32p

    def refused(fn, code=capi.ERR_INVALID):
        with pytest.raises(capi.VgxError) as e:
            fn()
        assert e.value.code == code, e.value

    # the configuration, at creation
    for kw in (dict(s_max=0.0), dict(min_step=0.0), dict(unknown_step=-1.0), dict(max_bracket=0.0), dict(s_min=-0.1), dict(s_min=7.0),
               dict(step_scale=0.0), dict(s_max=math.inf), dict(max_bracket=math.nan), dict(s_max=2000.0), dict(image_width=-1),
               dict(flags=32)):
        refused(lambda: capi.View(ctx, capi.view_config(**dict(CFG, **kw))))
    refused(lambda: capi.View(ctx, None))
    assert lib.vgx_view_create(ctx.h, capi.C.byref(capi.view_config(**CFG)), None) == capi.ERR_INVALID

    n = 200
    view = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **CFG))
    assert view.stats()["n_rays"] == 0 and view.device_pointers().range is None
    layer.render_view(view, T, dirs[:n])
    before, counts = view.download(), view.stats()
    sm = capi.Submap(ctx, 5, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.esdf_distance, d.esdf_observed)
    other = capi.Context(0)
    foreign_layer = capi.TsdfLayer(other, d.voxel_size, d.vps)
    foreign_view = capi.View(other, capi.view_config(**CFG))
    foreign_sm = capi.Submap(other, 6, d.voxel_size, d.vps, d.block_index, d.tsdf_distance, d.tsdf_weight, d.esdf_distance, d.esdf_observed)
    Tg, dg = capi._f32(T), np.ascontiguousarray(dirs[:n])
    nan_T, inf_T, long_T = Tg.copy(), Tg.copy(), Tg.copy()
    nan_T[5], inf_T[0] = np.nan, np.inf
    long_T[:4] *= F(1.0001)

    def calls(host, device, source, foreign):
        def run(src=source.h, v=view.h, T=Tg, n=n, dirs=dg):
            return host(src, v, capi._ptr(T, f32p), n, capi._ptr(dirs, f32p))
        return [run(src=None), run(T=None), run(dirs=None), run(n=-1), run(T=nan_T), run(T=inf_T), run(T=long_T),
                run(src=foreign.h), run(v=foreign_view.h), run(v=None),
                device(source.h, view.h, capi._ptr(Tg, f32p), n, None), device(None, view.h, capi._ptr(Tg, f32p), n, None)]

    for rc in (calls(lib.vgx_tsdf_layer_render_view, lib.vgx_tsdf_layer_render_view_device, layer, foreign_layer) +
               calls(lib.vgx_submap_render_view, lib.vgx_submap_render_view_device, sm, foreign_sm) +
               [lib.vgx_view_stats(view.h, None)]):
        assert rc == capi.ERR_INVALID
    # too many rays for one launch: refused before anything is read (an address nobody dereferences)
    assert lib.vgx_tsdf_layer_render_view_device(layer.h, view.h, capi._ptr(Tg, f32p), (2 ** 31 - 1) * 256 + 1, capi.vp(1 << 20)) == capi.ERR_UNSUPPORTED
    # nothing was written by any refused call: the view holds what it held
    assert view.stats() == counts
    for x, y in zip(before, view.download()):
        assert np.array_equal(_bits(x), _bits(y))
    # n = 0 is an answer: the view then holds no ray
    assert lib.vgx_tsdf_layer_render_view(layer.h, view.h, capi._ptr(Tg, f32p), 0, None) == capi.OK
    assert view.stats()["n_rays"] == 0 and len(view.download().range) == 0 and view.device_pointers().points is None
    assert lib.vgx_submap_render_view_device(sm.h, view.h, capi._ptr(Tg, f32p), 0, None) == capi.OK
    # a layer of another voxels_per_side cannot be made (vgx_tsdf_layer_create and vgx_submap_create refuse it), so that
    # refusal is unreachable
    refused(lambda: capi.TsdfLayer(ctx, 0.1, 4), capi.ERR_UNSUPPORTED)
    # an empty layer and an empty submap: every ray with a direction is a MISS
    empty = capi.TsdfLayer(ctx, d.voxel_size, d.vps)
    Lempty = V.layer_of(d.voxel_size, d.vps, np.zeros((0, 3), np.int32), np.zeros((0, d.vps ** 3), F), np.zeros((0, d.vps ** 3), F))
    got = _same(empty.render_view(view, T, dirs[:n]), V.render(Lempty, T, dirs[:n], V.config(**CFG)))
    assert set(np.unique(got.status)) == {capi.VIEW_MISS, capi.VIEW_BAD}
    for x in (empty, view, sm, foreign_sm, foreign_view, foreign_layer):
        x.destroy()
    other.close()


def test_special_voxel_values_fall_under_the_stated_comparisons(ctx):
    """One ray straight up through tests/special_voxel_scene.py's layer (D = Z0 - z), a special value planted into the
    cube CELL on its way.  The expectations are IEEE's under the header's rules, written down by hand:
    s_min puts the first sample in the cube below CELL (D = 0.11 > 0: have, s0 = s_min), the second falls into CELL."""
    from tests import special_voxel_scene as Z
    bi, d, w = Z.layer()
    T = np.array([1, 0, 0, 0, Z.X, Z.Y, -0.7], F)
    up = np.array([[0, 0, 1]], F)
    cfg = dict(s_min=0.5, s_max=1.4, min_step=0.025, unknown_step=0.1, max_bracket=0.2)
    bracketed = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **cfg))
    unbracketed = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **dict(cfg, s_min=0.58)))   # the first sample in CELL
    layer = capi.TsdfLayer(ctx, Z.VOXEL_SIZE, Z.VPS)

    def render(dd=d, ww=w, view=bracketed):
        layer.upload(bi, dd, ww)
        got = layer.render_view(view, T, up).download()
        return types.SimpleNamespace(status=int(got.status[0]), range=got.range[0], point=got.points[0], gradient=got.gradient[0],
                                     weight=got.weight[0], rgba=got.rgba[0], n_samples=int(got.n_samples[0]))

    def zero_bits(*arrays):
        return all(not np.ascontiguousarray(a).view(np.uint8).any() for a in arrays)

    nb7, cell, other = [Z.NEIGHBOUR_7], Z.CELL, [Z.CELL[1]]        # (CELL[1]: x 1, y 2, z 7 -- not in the cube below either)
    # nothing planted: samples at z = -0.2, -0.1175, -0.0925, -0.0675 (the first D < 0), the hit at z = Z0
    base = render()
    assert base.status == capi.VIEW_HIT and abs(base.range - 0.61) < 1e-3 and base.n_samples == 5 and base.weight == 1
    assert np.allclose(base.gradient, [0, 0, -1], atol=1e-3) and np.allclose(base.point, [0, 0, base.range])
    # weight 1e-40 (a denormal) and +inf are > 0: observed, the same march; the interpolated weight is the interpolant's
    for value in Z.WEIGHTS_OBSERVED:
        got = render(ww=Z.plant(bi, w, nb7, value))
        assert got.status == capi.VIEW_HIT and got.range.tobytes() == base.range.tobytes() and got.n_samples == 5, value
        assert (0 < got.weight < 1) if np.isfinite(value) else not np.isfinite(got.weight), (value, got.weight)
    # weight NaN, -0.0, 0.0, -1 are not > 0: every sample in CELL and in the cube above it (which holds neighbour 7 too) is
    # invalid and advances by unknown_step -- z = -0.1175, -0.0175 -- and the next valid one, z = 0.0825 with D < 0, lies
    # 0.2825 > max_bracket behind s0: INSIDE
    for value in Z.WEIGHTS_UNOBSERVED:
        got = render(ww=Z.plant(bi, w, nb7, value))
        assert got.status == capi.VIEW_INSIDE and got.n_samples == 4 and zero_bits(got.range, got.point, got.gradient, got.weight, got.rgba), value
    # distance NaN under valid weights is "not (D > 0)".  Bracketed: a hit whose range is s0 + gap * (D0 / (D0 - NaN)) = NaN;
    # the sample at a NaN position is invalid: HIT_UNSAMPLED, gradient / weight / rgba +0, the point dir * NaN.
    # An inf in neighbour 1 meets its own negation in the coefficients (c3 = +-inf, c5 = -+inf): the same NaN.
    for where, value in ((nb7, np.nan), (other, np.inf), (other, -np.inf)):
        got = render(Z.plant(bi, d, where, value))
        assert got.status == capi.VIEW_HIT_UNSAMPLED and np.isnan(got.range) and np.isnan(got.point).all() and got.n_samples == 3, value
        assert zero_bits(got.gradient, got.weight, got.rgba)
        # unbracketed (no positive sample before it): INSIDE
        got = render(Z.plant(bi, d, where, value), view=unbracketed)
        assert got.status == capi.VIEW_INSIDE and got.n_samples == 1 and zero_bits(got.range, got.point, got.gradient, got.weight, got.rgba)
    # distance +inf in neighbour 7 reaches D as +inf > 0: the step is inf, s = inf, and !(s <= s_max): MISS
    got = render(Z.plant(bi, d, nb7, np.inf))
    assert got.status == capi.VIEW_MISS and got.n_samples == 2 and zero_bits(got.range, got.point, got.gradient, got.weight, got.rgba)
    # distance -inf there reaches D as -inf, not > 0 and bracketed: s_hit = s0 + gap * (D0 / (D0 + inf)) = s0 + gap * 0 = s0
    # exactly -- the hit is reported AT the last positive sample, whose cube is clean: HIT, the field's gradient
    got = render(Z.plant(bi, d, nb7, -np.inf))
    assert got.status == capi.VIEW_HIT and got.range.tobytes() == F(0.5).tobytes() and got.n_samples == 3
    assert np.allclose(got.gradient, [0, 0, -1], atol=1e-3) and got.weight == 1
    # ... and unbracketed it is INSIDE, like every D that is not > 0
    assert render(Z.plant(bi, d, nb7, -np.inf), view=unbracketed).status == capi.VIEW_INSIDE
    # -0.0, 0.0 and 1e-40 in one neighbour are ordinary values: they flow through (added to a non-zero partial sum the
    # three give the same bits), the surface moves within CELL
    ranges = [render(Z.plant(bi, d, nb7, value)) for value in (-0.0, 0.0, 1e-40)]
    assert all(g.status == capi.VIEW_HIT and 0.55 < g.range < 0.65 for g in ranges)
    assert len({g.range.tobytes() for g in ranges}) == 1 and ranges[0].range != base.range
    # all 8 neighbours -0.0 (four of them are the upper face of the cube below: D0 = 0.08 there, the second sample at
    # z = -0.14): D is a zero, and a zero is "not > 0" whatever its sign: the hit at the second sample itself,
    # s_hit = s0 + gap * (D0 / (D0 - 0)) = s0 + gap
    got = render(Z.plant(bi, d, cell, -0.0))
    assert got.status == capi.VIEW_HIT and got.n_samples == 3 and abs(got.range - 0.56) < 1e-3
    # all 8 neighbours 1e-40: D = 1e-40 > 0, a positive distance like any other (a device that flushed denormals would see
    # the zero above).  The march goes on by min_step through CELL -- z = -0.14, -0.115, -0.09, -0.065 -- to z = -0.04 in the
    # cube above, D < 0; the hit lies a hair (1e-40 / 0.014 of the gap) past the last of them, z = -0.065
    got = render(Z.plant(bi, d, cell, 1e-40))
    assert got.status == capi.VIEW_HIT and got.n_samples == 7 and abs(got.range - 0.635) < 1e-3
    for x in (bracketed, unbracketed, layer):
        x.destroy()
