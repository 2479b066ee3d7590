"""Sequential restatement of view rendering (include/voxgraph_amd.h, "View rendering") in numpy f32 -- every
numpy op rounds once, as the kernel's do without contraction, in the kernel's order.  All rays advance together, one sample
per pass; a ray's arithmetic never depends on another's.  The sample is scan_registration_ref's (`_neighbours`,
`trilinear`, `trilinear_gradient`), the rotation projected_map_ref's, weight and colour at the hit map_colour_ref's
interpolation.  Test infrastructure: not part of the product."""
import types

import numpy as np

from tests import map_colour_ref as mc
from tests import scan_registration_ref as sr
from tests.projected_map_ref import F, quat_rotate

MISS, HIT, INSIDE, BAD, HIT_UNSAMPLED = range(5)
LIMIT = sr.LIMIT
MAX_SAMPLES = 1 << 17           # the kernel's loop bound (never reached: s_max / min step <= 65536)
COUNTS = ("n_rays", "n_hit", "n_hit_unsampled", "n_miss", "n_inside", "n_bad", "n_samples")

View = types.SimpleNamespace


def config(s_max, min_step, unknown_step, max_bracket, s_min=0.0, step_scale=0.75):
    return types.SimpleNamespace(s_min=F(s_min), s_max=F(s_max), step_scale=F(step_scale), min_step=F(min_step),
                                 unknown_step=F(unknown_step), max_bracket=F(max_bracket))


def layer_of(voxel_size, vps, block_index, distance, weight, rgba=None):
    """scan_registration_ref.layer_of with the voxels' colours ([n][vps^3][4] u8, or None): a map_colour_ref.ColourLayer"""
    raw = sr.layer_of(voxel_size, vps, block_index, distance, weight)
    return mc.ColourLayer(types.SimpleNamespace(vps=vps, voxel_size=voxel_size, block_index=raw.bi, tsdf_distance=raw.d,
                                                tsdf_weight=raw.w, tsdf_rgba=rgba))


def _sample(L, p):
    """one sample at positions [m][3] f32 -> (valid [m], (d8, dl) of scan_registration_ref._neighbours)"""
    with np.errstate(all="ignore"):
        inside = (np.abs((p * L.bs_inv).astype(F)) < F(LIMIT)).all(1)
    p = np.where(inside[:, None], p, F(0)).astype(F)        # (kept out of the integer casts; masked by `inside`)
    ok, d8, dl = sr._neighbours(L, p, F)
    return inside & ok, d8, dl, p


def render(L, T, dirs, cfg):
    """vgx_*_render_view -> View(range, status, points, gradient, weight, rgba [n][4] u8, n_samples, counts dict)"""
    dirs = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = len(dirs)
    T = np.asarray(T, F).reshape(7)
    o = T[4:7]
    status = np.full(n, MISS, np.uint8)
    rng, points, gradient = np.zeros(n, F), np.zeros((n, 3), F), np.zeros((n, 3), F)
    weight, rgba, samples = np.zeros(n, F), np.zeros((n, 4), np.uint8), np.zeros(n, np.int32)
    bad = ~np.isfinite(dirs).all(1) | (dirs == 0).all(1)
    status[bad] = BAD
    with np.errstate(all="ignore"):
        d = quat_rotate(T[:4], np.where(bad[:, None], F(0), dirs).astype(F))
        s = np.full(n, cfg.s_min, F)
        s0, D0 = np.zeros(n, F), np.zeros(n, F)
        have, hit, active = np.zeros(n, bool), np.zeros(n, bool), ~bad
        for _ in range(MAX_SAMPLES):
            active &= s <= cfg.s_max                        # 1. (a ray that leaves here stays a MISS)
            idx = np.nonzero(active)[0]
            if not len(idx):
                break
            si = s[idx]
            p = ((d[idx] * si[:, None]).astype(F) + o).astype(F)   # 2. a multiply, then an add
            samples[idx] += 1
            ok, d8, dl, _ = _sample(L, p)                   # 3.
            D = sr.trilinear(d8, dl).astype(F)              # 4.
            pos, neg = ok & (D > F(0)), ok & ~(D > F(0))
            i = idx[pos]
            have[i], s0[i], D0[i] = True, si[pos], D[pos]
            step = (D[pos] * cfg.step_scale).astype(F)
            s[i] = (si[pos] + np.where(step > cfg.min_step, step, cfg.min_step).astype(F)).astype(F)
            i = idx[neg]
            gap = (si[neg] - s0[i]).astype(F)
            is_hit = have[i] & (gap <= cfg.max_bracket)
            rng[i] = np.where(is_hit, (s0[i] + (gap * (D0[i] / (D0[i] - D[neg]).astype(F)).astype(F)).astype(F)).astype(F), F(0))
            hit[i] = is_hit
            status[i] = np.where(is_hit, HIT_UNSAMPLED, INSIDE)   # (a hit becomes HIT below, where its sample is valid)
            active[i] = False
            i = idx[~ok]
            s[i] = (si[~ok] + cfg.unknown_step).astype(F)
        else:
            raise AssertionError("a ray took MAX_SAMPLES samples")
        idx = np.nonzero(hit)[0]
        if len(idx):
            sh = rng[idx]
            p = ((d[idx] * sh[:, None]).astype(F) + o).astype(F)
            points[idx] = (dirs[idx] * sh[:, None]).astype(F)
            samples[idx] += 1
            ok, d8, dl, pm = _sample(L, p)
            g = sr.trilinear_gradient(d8, dl)
            _, _, w, c, _ = L.interp_coloured(pm)
            i = idx[ok]
            status[i] = HIT
            gradient[i] = np.stack([(ga * L.vs_inv).astype(F) for ga in g], -1)[ok]
            weight[i] = w[ok]
            rgba[i] = c[ok]
    counts = dict(n_rays=n, n_hit=int((status == HIT).sum()), n_hit_unsampled=int((status == HIT_UNSAMPLED).sum()),
                  n_miss=int((status == MISS).sum()), n_inside=int((status == INSIDE).sum()), n_bad=int((status == BAD).sum()),
                  n_samples=int(samples.sum(dtype=np.int64)))
    return View(range=rng, status=status, points=points, gradient=gradient, weight=weight, rgba=rgba, n_samples=samples, counts=counts)


def rays_pinhole(width, height, fx, fy, cx, cy):
    """vgx_view_rays_pinhole in numpy f64, rounded to f32 once"""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    x, y = (u - cx) / fx, (v - cy) / fy
    norm = np.sqrt((x * x + y * y) + 1.0)
    return np.stack([x / norm, y / norm, 1.0 / norm], -1).reshape(-1, 3).astype(F)


def rays_lidar(width, height, elevation_min, elevation_max, azimuth_offset=0.0):
    """vgx_view_rays_lidar in numpy f64, rounded to f32 once"""
    r, c = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    el = elevation_min + r * (elevation_max - elevation_min) / (height - 1) if height > 1 else np.full_like(r, elevation_min)
    az = (-np.pi + azimuth_offset) + c * (2.0 * np.pi) / width
    return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3).astype(F)


def room_dirs(n_az=256, n_el=16):
    """the unit directions of scan_registration_ref.room_scan's beams [n_el n_az][3] f32, by its own expressions
    (rays_lidar(n_az, n_el, -0.296, 0.304, (2 pi / n_az) / 3) is the same within an ulp)"""
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, n_az, endpoint=False) + (2 * np.pi / n_az) / 3.0,
                         np.linspace(-0.3, 0.3, n_el) + 0.004)
    return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3).astype(F)

