"""The scene generator of the layer readers' fuzzer (profiles/fuzz_layer_readers.py: view rendering, scan-to-map
registration, scan localisation) and of tests/test_fuzz_readers_cpu.py.  numpy, oracle/synth.py and the helpers of
profiles/fuzz_map_scene.py only: importable without a GPU and without the library.

draw(seed) gives one scene from one np.random.default_rng([seed, TAG]) (a stream of its own: fuzz_map_scene.draw's
scenes do not change).  The categorical classes follow the seed round robin, so that a short run of consecutive seeds
draws each of them; everything else comes from the generator.  scene.drawn reports the classes a seed drew.

Geometry: fuzz_map_scene's.  Every block box lies around one common block offset, on one seed in four up to 2^20 blocks
from the origin on some axes (f32 coordinates of millions of metres: a sample point is then a coarse grid point, index
arithmetic at its limits; the restatement's block key holds 21 bits per axis, so the offset stays 4096 blocks inside
that).  The live layer's frame is the mission frame; a submap's pose is a rotation about the scene's centre plus a small
shift, so that the posed submaps and the live layer overlap wherever the offset is.

Value kind `specials`: a noise scene in which about 2 % of the voxels carry a special DISTANCE (NaN, +-inf, +-0.0, a
denormal of either sign, 3e38) and, drawn independently, about 2 % a special WEIGHT (NaN, +inf, +-0.0, -1, the
denormals 1e-40 and 1e-45) -- the values at which the readers' comparisons ("all 8 weights > 0", "not (D > 0)",
"|D| < max_abs_distance_m") are decided by IEEE alone.  scene.planted holds where each was put."""
import types

import numpy as np

from oracle import synth
from profiles import fuzz_map_scene as S

F = np.float32
TAG = 0x7264
VALUE_KINDS = S.VALUE_KINDS + ("specials",)
DISTANCE_SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 3e38]).astype(F)
WEIGHT_SPECIALS = np.array([np.nan, np.inf, -0.0, 0.0, -1.0, 1e-40, 1e-45]).astype(F)
SPECIAL_FRACTION = 0.02
N_SUBMAPS = (1, 2, 3, 5)
POINT_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 4097)
STRIDES = (1, 2, 3)
N_POSES = (1, 2, 7, 65)
RAY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
IMAGES = ((1, 1), (7, 5), (8, 8), (9, 17), (64, 16), (65, 9))             # (width, height)
LAYERS = ("esdf", "tsdf")
FAR_LIMIT = (1 << 20) - 4096
MAX_VIEW_PASSES = 512                    # s_max / min(min_step, unknown_step): the restatement's loop stays short
MAX_ITERATIONS = (1, 3, 8)


def plant_specials(rng, a, specials):
    """about SPECIAL_FRACTION of a's elements replaced, in place, by draws from `specials` -> int8 array of a's shape:
    the index of the special planted there, -1 where none was"""
    which = np.full(a.shape, -1, np.int8)
    mask = rng.random(a.shape) < SPECIAL_FRACTION
    pick = rng.integers(0, len(specials), int(mask.sum()))
    a[mask] = specials[pick]
    which[mask] = pick
    return which


def _box(rng, offset, roomy):
    """(block_index, shape kind) of one layer around `offset`; roomy: the live layer's box is never a single block wide"""
    shape = S.SHAPE_KINDS[int(rng.choice(3, p=[0.7, 0.15, 0.15]))]
    if shape == "one_block":
        dims = np.ones(3, np.int64)
    elif shape == "slab":
        dims = np.ones(3, np.int64)
        dims[rng.integers(0, 3)] = rng.integers(2, 5)
    else:
        dims = rng.integers(2 if roomy else 1, 5, 3)
    lo = offset + rng.integers(-1, 2, 3) - (dims - 2) // 2
    return S._block_box(rng, lo, dims, rng.uniform(0.3, 1.0)), shape


def _tsdf(rng, kind, T, bi, vs, vps, centre):
    """distance, weight and the planted specials (None unless kind is `specials`) of a layer posed at T (None: identity)"""
    c = synth.voxel_centres(vs, vps, bi).astype(np.float64)
    world = c if T is None else S._transform64(T, c.reshape(-1, 3)).reshape(c.shape)
    # (the sphere and the ground of the analytic kinds are placed about the middle of this layer's own box, so that the
    # surface passes through the layer however small it is: a truncated layer without a surface has no observed voxel)
    middle = 0.5 * (bi.min(0) + bi.max(0) + 1.0) * (vs * vps)
    middle = middle if T is None else S._transform64(T, middle[None])[0]
    d, w = S._values(rng, "noise" if kind == "specials" else kind, world, vs, vps, middle)
    S.plant_edges(rng, d, w, 1.0)
    planted = None
    if kind == "specials":
        planted = (plant_specials(rng, d, DISTANCE_SPECIALS), plant_specials(rng, w, WEIGHT_SPECIALS))
    return d, w, planted


def _sensor_position(rng, bi, d, w, vs, vps):
    """(a point of the layer's frame to look from, a point to look at): next to the centre of an observed voxel just in
    front of the surface (0.5 voxel < D < 2.5 voxels where there is one, else 0.5 voxel < D) and the centre of the nearest
    observed voxel behind it -- rays then start in known free space next to the surface and most views hold a HIT.  A
    layer without such voxels: anywhere in its box, looking at its middle."""
    c = synth.voxel_centres(vs, vps, bi).astype(np.float64)
    bs = vs * vps
    lo, hi = bi.min(0) * bs, (bi.max(0) + 1) * bs
    with np.errstate(invalid="ignore"):
        seen = (w > 0) & np.isfinite(d)
        front = seen & (d > F(0.5 * vs)) & (d < F(1e30))
        near = front & (d < F(2.5 * vs))
        behind = np.argwhere(seen & (d < 0))
    good = np.argwhere(near if near.any() else front)
    if not len(good):
        return rng.uniform(lo, hi), 0.5 * (lo + hi)
    b, v = good[int(rng.integers(0, len(good)))]
    pos = c[b, v] + rng.uniform(-0.3, 0.3, 3) * vs
    if not len(behind):
        return pos, 0.5 * (lo + hi)
    cb = c[behind[:, 0], behind[:, 1]]
    return pos, cb[int(np.argmin(((cb - pos) ** 2).sum(1)))]


def _aim(dirs, i, q, pos, target):
    """dirs[i] = the sensor-frame direction from pos to target (layer frame), unit in f64 and rounded once"""
    v = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    n = np.linalg.norm(v)
    if n > 0:
        dirs[i] = (S._quat_matrix(np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))).T @ (v / n)).astype(F)


def _directions(rng, n):
    """[n][3] f32: random directions, one in seven not unit (the library never normalises), 2 % non-finite or zero"""
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs[::7] *= rng.uniform(0.3, 3.0, (len(dirs[::7]), 1))
    dirs = dirs.astype(F)
    bad = rng.random(n) < 0.02
    dirs[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum())).astype(F)
    dirs[rng.random(n) < 0.005] = F(0)
    return np.ascontiguousarray(dirs)


def _view_config(rng, vs, bs):
    """view_render_ref.config's keywords in voxels and blocks, s_max cut so that the march takes at most MAX_VIEW_PASSES
    passes (as the library forms the ratio: in f64 from the f32 fields)"""
    min_step = float(F(rng.uniform(0.15, 0.5) * vs))
    unknown_step = float(F(rng.uniform(0.5, 1.5) * vs))
    s_max = float(F(min(rng.uniform(1.5, 4.0) * bs, 0.95 * MAX_VIEW_PASSES * min(min_step, unknown_step))))
    assert s_max / min(min_step, unknown_step) <= MAX_VIEW_PASSES
    return dict(s_max=s_max, min_step=min_step, unknown_step=unknown_step, max_bracket=float(F(rng.uniform(2.0, 4.0) * vs)),
                s_min=float(F(rng.choice([0.0, 0.0, rng.uniform(0.0, 1.0) * vs]))), step_scale=float(rng.choice([0.75, 0.5, 1.0])))


def _typical_distance(d, w):
    """the 90th percentile of |D| over the observed voxels with a finite distance (the value range `max_abs_distance_m` is
    drawn against); 1.0 where there is none"""
    with np.errstate(invalid="ignore"):
        ok = (w > 0) & np.isfinite(d) & (np.abs(d) < F(1e30))
    return float(np.percentile(np.abs(d[ok]), 90)) if ok.any() else 1.0


def draw(seed):
    from tests import scan_localization_scenes as LS
    from tests.projected_map_ref import inverse, quat_rotate
    rng = np.random.default_rng([seed, TAG])
    vps = int(rng.choice([8, 16]))
    vs = float(F(S.VOXEL_SIZES[seed % len(S.VOXEL_SIZES)]))
    bs = float(F(F(vps) * F(vs)))
    nv = vps ** 3
    value_kind = VALUE_KINDS[seed % len(VALUE_KINDS)]
    far = seed % 4 == 1
    offset = rng.integers(-40, 41, 3) * (rng.random(3) < 0.85)
    if far:
        axes = rng.random(3) < 0.6
        axes[rng.integers(0, 3)] = True
        mag = np.minimum(1 << rng.integers(8, 21, 3), FAR_LIMIT) - rng.integers(0, 64, 3)
        offset = np.where(axes, rng.choice([-1, 1], 3) * mag, offset)
    centre = (offset + 1.0) * bs

    # the live layer: the mission frame
    live_bi, live_shape = _box(rng, offset, True)
    live_d, live_w, live_planted = _tsdf(rng, value_kind, None, live_bi, vs, vps, centre)
    live_rgba = rng.integers(0, 256, (len(live_bi), nv, 4), dtype=np.uint8)

    # K posed finished submaps, every one with a TSDF and a drawn (not generated) ESDF
    K = N_SUBMAPS[(seed + seed // 5) % len(N_SUBMAPS)]
    first_kind = S.POSE_KINDS[(seed + seed // 6) % len(S.POSE_KINDS)]
    subs, poses, pose_kinds, shapes, planted = [], [], [], [], []
    for k in range(K):
        bi, shape = _box(rng, offset, False)
        kind = first_kind if k == 0 else S.POSE_KINDS[int(rng.integers(0, len(S.POSE_KINDS)))]
        T = S.draw_pose(rng, kind, centre, vs)
        td, tw, tp = _tsdf(rng, value_kind, T, bi, vs, vps, centre)
        ed = rng.uniform(-0.5, 0.5, (len(bi), nv)).astype(F)
        eo = (rng.random((len(bi), nv)) < 0.9).astype(np.uint8)
        ep = plant_specials(rng, ed, DISTANCE_SPECIALS) if value_kind == "specials" else None
        subs.append(synth.SubmapData(vs, vps, bi, td, tw, ed, eo, np.zeros(4)))
        poses.append(T)
        pose_kinds.append(kind)
        shapes.append(shape)
        planted.append(None if tp is None else dict(tsdf_distance=tp[0], tsdf_weight=tp[1], esdf_distance=ep))
    # the list handed to set_map: indices into subs (-1: a submap of zero blocks); one seed in four lists an empty submap,
    # one in four lists one submap twice (its second entry under a pose of its own)
    listed = list(range(K))
    listed_poses = list(poses)
    empty, duplicate = seed % 4 == 2, seed % 4 == 3
    if empty:
        at = int(rng.integers(0, len(listed) + 1))
        listed.insert(at, -1)
        listed_poses.insert(at, S.draw_pose(rng, "full", centre, vs))
    if duplicate:
        at, k = int(rng.integers(0, len(listed) + 1)), int(rng.integers(0, K))
        listed.insert(at, k)
        listed_poses.insert(at, S.draw_pose(rng, S.POSE_KINDS[int(rng.integers(0, len(S.POSE_KINDS)))], centre, vs))
    listed_poses = np.stack(listed_poses).astype(F)

    # the sensor: a rotation of a drawn kind, a position in front of the live layer's surface
    sensor_kind = S.POSE_KINDS[(seed + seed // 6 + 2) % len(S.POSE_KINDS)]
    q = S.draw_pose(rng, sensor_kind, centre, vs)[:4]
    live_pos, live_target = _sensor_position(rng, live_bi, live_d, live_w, vs, vps)
    T_sensor = np.array([*q, *live_pos], F)
    view_submap = int(rng.integers(0, K))
    vsm = subs[view_submap]
    sub_pos, sub_target = _sensor_position(rng, vsm.block_index, vsm.tsdf_distance, vsm.tsdf_weight, vs, vps)
    T_view_submap = np.array([*q, *sub_pos], F)
    submap_rgba = rng.integers(0, 256, (len(vsm.block_index), nv, 4), dtype=np.uint8) if seed % 2 == 0 else None

    # rays: an image (image_width its width) or an unorganised set (launched a second time under a drawn width)
    organised = (seed // 2) % 2 == 0
    if organised:
        width, height = IMAGES[(seed + seed // 6) % len(IMAGES)]
        n_rays = width * height
    else:
        n_rays = RAY_SIZES[(seed + seed // 8 + 3) % len(RAY_SIZES)]
        width, height = int(rng.choice([1, 7, 8, 9, 64])), 0
    dirs = _directions(rng, n_rays)
    _aim(dirs, n_rays - 1, q, sub_pos, sub_target)               # one ray that looks at each layer's surface (a view of one
    _aim(dirs, 0, q, live_pos, live_target)                      # ray looks at the live layer's)
    view_cfg = _view_config(rng, vs, bs)

    # sensor-frame points: every kind of point of the live layer and of every submap with a block, through the poses into
    # the mission frame and back through the sensor pose; 2 % non-finite
    n_points = POINT_SIZES[(seed + seed // 8) % len(POINT_SIZES)]
    sources = [(synth.SubmapData(vs, vps, live_bi, live_d, live_w, None, None, np.zeros(4)), S.IDENT)] + list(zip(subs, poses))
    per = -(-n_points // len(sources))
    pm = np.concatenate([(quat_rotate(T[:4], LS._submap_points(rng, d, per)) + T[4:]).astype(F) for d, T in sources])
    pm = pm[rng.permutation(len(pm))][:n_points]
    qi, ti = inverse(T_sensor)
    points = (quat_rotate(qi, pm) + ti).astype(F)
    bad = rng.random(len(points)) < 0.02
    points[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf, 3e38], int(bad.sum())).astype(F)
    points = np.ascontiguousarray(points, F)
    assert len(points) == n_points

    # scan-to-map registration on the live layer
    point_stride = STRIDES[seed % len(STRIDES)]
    reg_cfg = dict(max_abs_distance_m=float(F(rng.uniform(0.5, 1.5) * _typical_distance(live_d, live_w))), point_stride=point_stride,
                   min_valid_ratio=float(F(rng.choice([0.02, 0.1, 0.3]))), min_range_m=float(F(rng.choice([0.0, 0.5 * vs]))),
                   max_range_m=float(F(rng.choice([np.inf, 6.0 * bs]))))
    delta = [*(rng.uniform(-1.0, 1.0, 3) * vs), float(rng.uniform(-0.05, 0.05))]
    max_iterations = MAX_ITERATIONS[seed % len(MAX_ITERATIONS)]

    # scan localisation on the listed submaps
    layer = LAYERS[(seed + seed // 4) % 2]
    huber = float("inf") if (seed // 2 + seed // 8) % 2 == 0 else float(F(rng.uniform(0.3, 2.0) * vs))
    score_point_stride = STRIDES[(seed // 3) % len(STRIDES)]
    if layer == "esdf":
        typical = 0.45                                                            # uniform(-0.5, 0.5): the 90th percentile of |D|
    else:
        typical = float(np.median([_typical_distance(s.tsdf_distance, s.tsdf_weight) for s in subs]))
    unreachable = seed % 16 == 5                                                   # a ratio no scan reaches: no hypothesis is eligible
    loc_cfg = dict(max_abs_distance_m=float(F(rng.uniform(0.5, 1.5) * typical)), point_stride=point_stride,
                   min_valid_ratio=float(F(0.999 if unreachable else rng.choice([0.005, 0.02, 0.05]))))
    map_cfg = dict(layer=layer, huber_delta_m=huber, score_point_stride=score_point_stride)
    n_poses = N_POSES[(seed + seed // 4) % len(N_POSES)]
    hyp = []
    for m in range(n_poses):
        near = np.array([1, *(rng.normal(size=3) * 0.01), *(rng.uniform(-1.5, 1.5, 3) * vs)])
        near[:4] /= np.linalg.norm(near[:4])
        hyp.append(LS.compose(T_sensor, near.astype(F)))
    hyp = np.array(hyp, F)
    hyp[:, :4] = (hyp[:, :4].astype(np.float64) / np.linalg.norm(hyp[:, :4].astype(np.float64), axis=1)[:, None]).astype(F)
    scored = np.arange(n_poses) if n_poses <= 7 else np.sort(rng.choice(n_poses, 8, replace=False))
    loc_delta = [*(rng.uniform(-0.5, 0.5, 3) * vs), float(rng.uniform(-0.03, 0.03))]

    drawn = {"value_kind": {value_kind}, "vps": {vps}, "voxel_size": {vs}, "far_box": {bool(far)}, "pose_kind": set(pose_kinds) | {sensor_kind},
             "shape": set(shapes) | {live_shape}, "n_submaps": {K}, "empty_submap": {empty}, "duplicate": {duplicate}, "layer": {layer},
             "huber_finite": {bool(np.isfinite(huber))}, "point_stride": {point_stride}, "score_point_stride": {score_point_stride},
             "n_points": {n_points}, "n_poses": {n_poses}, "rays": {("image", width, height) if organised else ("rays", n_rays)},
             "max_iterations": {max_iterations}, "unreachable_ratio": {unreachable}}
    return types.SimpleNamespace(
        seed=seed, vps=vps, voxel_size=vs, block_size=bs, value_kind=value_kind, offset=offset, centre=centre, far=far,
        live=(live_bi, live_d, live_w, live_rgba), live_shape=live_shape, live_planted=live_planted, subs=subs, poses=np.stack(poses).astype(F),
        pose_kinds=pose_kinds, shapes=shapes, planted=planted, listed=listed, listed_poses=listed_poses, sensor_kind=sensor_kind,
        T_sensor=T_sensor, view_submap=view_submap, T_view_submap=T_view_submap, submap_rgba=submap_rgba, organised=organised,
        image=(width, height), dirs=dirs, view_cfg=view_cfg, points=points, reg_cfg=reg_cfg, delta=delta, max_iterations=max_iterations,
        loc_cfg=loc_cfg, map_cfg=map_cfg, hyp=hyp, scored=scored, loc_delta=loc_delta, drawn=drawn, rng=rng)


def empty_submap(sc):
    """the listed submap of zero blocks"""
    nv = sc.vps ** 3
    return synth.SubmapData(sc.voxel_size, sc.vps, np.zeros((0, 3), np.int32), np.zeros((0, nv), F), np.zeros((0, nv), F),
                            np.zeros((0, nv), F), np.zeros((0, nv), np.uint8), np.zeros(4))


def listed_submaps(sc):
    """the SubmapData of set_map's list, in its order"""
    return [sc.subs[k] if k >= 0 else empty_submap(sc) for k in sc.listed]


def describe(sc):
    """the drawn configuration in one line, for a mismatch report"""
    rays = f"image {sc.image[0]}x{sc.image[1]}" if sc.organised else f"{len(sc.dirs)} rays (second launch: width {sc.image[0]})"
    return (f"seed {sc.seed}: vps {sc.vps} voxel_size {sc.voxel_size!r} values {sc.value_kind} offset {sc.offset.tolist()}"
            f"{' (far)' if sc.far else ''} live {len(sc.live[0])} blocks ({sc.live_shape}) submaps "
            f"{[(len(s.block_index), k, sh) for s, k, sh in zip(sc.subs, sc.pose_kinds, sc.shapes)]} listed {sc.listed} "
            f"sensor {sc.sensor_kind} {sc.T_sensor.tolist()} view of submap {sc.view_submap} {'coloured' if sc.submap_rgba is not None else 'plain'} "
            f"{rays} view {sc.view_cfg} points {len(sc.points)} registration {sc.reg_cfg} delta {sc.delta} max_iterations {sc.max_iterations} "
            f"localisation {sc.loc_cfg} {sc.map_cfg} delta {sc.loc_delta} hypotheses {len(sc.hyp)} scored {sc.scored.tolist()}")
