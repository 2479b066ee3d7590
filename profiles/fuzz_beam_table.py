"""Fuzz of the beam-table range image and its projective integration (vgx_range_image_build_beams,
vgx_tsdf_integrate_range_image on a table image; voxgraph_amd/csrc/vgx_range_image.hip) against the numpy restatement
(tests/beam_table_ref.py): random heights 1 .. 40 (a single row only under a finite limit), random monotone tables with
gaps of at least 1e-3 rad in either direction, offsets within +-0.1 rad with an occasional +-pi/2, a random limit or inf,
random poses and configurations, planted equal ranges, seam and zero-length points, two scans from nearby poses into one
layer, through a decoded scan and through device arrays in turn.  Every scene is compared bit for bit, as
profiles/fuzz_range_image.py compares.

    python profiles/fuzz_beam_table.py [first_seed [n_scenes]]        (needs the GPU; seeds 0 .. 99 run in the suite)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.fuzz_range_image import build, same_image, same_layer  # noqa: E402,F401
from tests import beam_table_ref as B  # noqa: E402

F = np.float32


def model(rng):
    """a random table sensor the check accepts"""
    width = int(rng.integers(16, 97))
    height = int(rng.integers(1, 41))
    limit = float(rng.uniform(0.004, 0.08)) if height == 1 or rng.random() < 0.5 else np.inf
    # (gaps of at most 0.12 rad, and a span of at most 1.4 rad: the candidate box grows by reach times the largest extent)
    gaps = np.maximum(rng.uniform(0.0, 1.0, max(height - 1, 0)) ** 2 * 0.12, 1e-3)
    if gaps.sum() > 1.4:
        gaps *= 1.4 / gaps.sum()
        gaps = np.maximum(gaps, 1e-3)
    mid = float(rng.uniform(-0.7, 0.7)) * (1.0 - gaps.sum() / 1.5)
    el = mid - 0.5 * gaps.sum() + np.concatenate([[0.0], np.cumsum(gaps)])
    if rng.random() < 0.5:
        el = el[::-1]
    off = rng.uniform(-0.1, 0.1, height)
    if rng.random() < 0.2:
        off[int(rng.integers(0, height))] = float(rng.choice([-1, 1])) * float(B.PI_2)
    az = float(rng.uniform(-1, 1) * float(B.PI)) if rng.random() < 0.8 else float(rng.choice([-1, 1]) * B.PI)
    m = B.BeamModel(width, el, None if rng.random() < 0.15 else off, az, int(rng.random() < 0.5), limit)
    assert m.check() == B.OK, (el, limit)
    return m


def scene(seed):
    """-> (BeamModel, scans [(pose, points, rgba)], Config, voxel size, vps): needs no device"""
    rng = np.random.default_rng(seed)
    m = model(rng)
    width, height = m.width, m.height
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.1, 0.2]))
    max_ray = float(rng.uniform(1.2, 2.5))
    cfg = B.Config(default_truncation_distance=float(vs * rng.uniform(1.5, 3.0)), max_weight=float(rng.choice([2.5, 10000.0])),
                   voxel_carving_enabled=int(rng.random() < 0.7), min_ray_length_m=float(rng.uniform(0.0, 0.5)),
                   max_ray_length_m=max_ray, use_const_weight=int(rng.random() < 0.4), allow_clear=int(rng.random() < 0.7),
                   use_weight_dropoff=int(rng.random() < 0.7))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    t = rng.uniform(-1, 1, 3) * float(rng.choice([1.0, 30.0, 400.0]))
    e_lo, e_hi = float(m.lo[0]), float(m.hi[-1])
    scans = []
    for k in range(2):
        v, u = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
        jitter = float(rng.choice([0.0, 0.3, 0.9]))          # (0.9 of a column; in elevation up to 1.3 half extents: into holes)
        lo, hi = m.extent(v)
        e = m.row_elevation_rad.astype(np.float64)[v]
        d_el = rng.uniform(-jitter, jitter, u.shape) * 1.45 * np.minimum(e - lo, hi - e)
        dirs = m.direction(u + rng.uniform(-jitter, jitter, u.shape), v, d_el).reshape(-1, 3)
        # a smooth surface between 0.3 and 1.6 max_ray, with noise
        r = max_ray * (0.95 + 0.65 * np.sin(u * rng.uniform(0.05, 0.4) + rng.uniform(0, 6)) * np.cos(v * rng.uniform(0.05, 0.4)))
        r = np.abs(r + rng.normal(0, 0.01, r.shape)).reshape(-1) + 0.05
        pts = (dirs * r[:, None]).astype(F)
        pts = pts[rng.random(len(pts)) > 0.08]                 # holes
        pts = pts[rng.permutation(len(pts))]
        n_dup = max(1, len(pts) // 10)
        dup = pts[rng.integers(0, len(pts), n_dup)]             # planted equal ranges: the same point again
        zr = rng.uniform(0.3, 2.0, 6)
        seam = np.stack([-zr, rng.choice([0.0, -0.0, 1e-7, -1e-7, 1e-3, -1e-3], 6), zr * np.tan(rng.uniform(e_lo, e_hi, 6))], 1)
        junk = np.array([[0, 0, 0], [0, 0, 1], [0, 0, -2], [-0.0, 0.0, -0.0]])
        pts = np.concatenate([pts, dup, seam.astype(F), junk.astype(F)]).astype(F)
        pts = pts[rng.permutation(len(pts))]
        rgba = rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)
        dq = np.concatenate([[1.0], rng.normal(0, 0.05 * k, 3)])
        qk = np.array([q[0] * dq[0] - q[1:] @ dq[1:], *(q[0] * dq[1:] + dq[0] * q[1:] + np.cross(q[1:], dq[1:]))])
        T = np.concatenate([qk / np.linalg.norm(qk), t + rng.normal(0, 0.1 * k, 3)]).astype(F)
        scans.append((T, pts, rgba))
    return m, scans, cfg, vs, vps


def run(capi, ctx, seed):
    """one scene on the device against the restatement -> (what differed or None, the frames' counts)"""
    m, scans, cfg, vs, vps = scene(seed)
    ref = B.Layer(vs, vps)
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, cfg.capi(capi), layer)
    image = capi.RangeImage(ctx)
    bad, all_counts = None, []
    try:
        for k, (T, pts, rgba) in enumerate(scans):
            want_img = B.build(m, pts, rgba)
            want = B.integrate(ref, T, want_img, cfg).counts
            got_img = build(capi, ctx, image, m, pts, rgba, (seed + k) % 2 == 0)
            if not B.same_counts(got_img, want_img.counts):
                bad = bad or f"scan {k}: image counts {got_img} != {want_img.counts}"
            what = same_image(image.download(), want_img)
            if what:
                bad = bad or f"scan {k}: the image's {what} differs"
            got = integ.integrate_range_image(T, image)
            all_counts.append(got)
            if got != want:
                bad = bad or f"scan {k}: counts {got} != {want}"
        bad = bad or same_layer(layer.download(), ref.download())
    finally:
        image.destroy()
        integ.destroy()
        layer.destroy()
    return bad, all_counts


def main():
    from voxgraph_amd import capi
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    ctx = capi.Context(0)
    failed, totals = [], dict(n_candidate_blocks=0, n_new_blocks=0, n_updates=0, n_carved=0, n_cleared=0)
    for seed in range(first, first + n):
        bad, counts = run(capi, ctx, seed)
        for c in counts:
            for k in totals:
                totals[k] += c[k]
        if bad:
            failed.append((seed, bad))
            print(f"seed {seed}: {bad}", flush=True)
    ctx.close()
    print(f"fuzz_beam_table: seeds {first}..{first + n - 1}, {n} scenes of two scans, {len(failed)} differ; totals {totals}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
