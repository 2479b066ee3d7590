"""Fuzz of the LiDAR range image and its projective integration (vgx_range_image_build, vgx_tsdf_integrate_range_image,
voxgraph_amd/csrc/vgx_range_image.hip) against the numpy restatement (tests/range_image_ref.py): random models, poses,
configurations and rooms, planted equal ranges, seam points and zero-length points, two scans from nearby poses into one
layer, through a decoded scan and through device arrays in turn.  Every scene is compared bit for bit: the image's ranges,
colours and winning indices, its counts, and the layer's distance, weight, colour, block index in slot order and the five
counts of each frame.

    python profiles/fuzz_range_image.py [first_seed [n_scenes]]        (needs the GPU; seeds 0 .. 99 run in the suite)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.fuzz_projective import same_layer  # noqa: E402
from tests import range_image_ref as R  # noqa: E402
from tests import range_image_scenes as S  # noqa: E402

F = np.float32


def scene(seed):
    """-> (Model, scans [(pose, points, rgba)], Config, voxel size, vps): needs no device"""
    rng = np.random.default_rng(seed)
    # (pitches of at most 0.4 and 0.12 rad: the candidate box grows by reach times their sum on every side)
    width, height = int(rng.integers(16, 97)), int(rng.integers(2, 25))
    half = min(0.5 * float(rng.uniform(0.02, 0.12)) * (height - 1), 0.7)
    mid = float(rng.uniform(-0.7, 0.7))
    e0, e1 = (mid - half, mid + half) if rng.random() < 0.5 else (mid + half, mid - half)
    m = R.Model(width, height, float(rng.uniform(-1, 1) * float(R.PI)) if rng.random() < 0.8 else float(rng.choice([-1, 1]) * R.PI),
                int(rng.random() < 0.5), e0, e1)
    assert m.check() == R.OK
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.1, 0.2]))
    max_ray = float(rng.uniform(1.2, 2.5))
    cfg = R.Config(default_truncation_distance=float(vs * rng.uniform(1.5, 3.0)), max_weight=float(rng.choice([2.5, 10000.0])),
                   voxel_carving_enabled=int(rng.random() < 0.7), min_ray_length_m=float(rng.uniform(0.0, 0.5)),
                   max_ray_length_m=max_ray, use_const_weight=int(rng.random() < 0.4), allow_clear=int(rng.random() < 0.7),
                   use_weight_dropoff=int(rng.random() < 0.7))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    t = rng.uniform(-1, 1, 3) * float(rng.choice([1.0, 30.0, 400.0]))
    scans = []
    for k in range(2):
        v, u = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
        jitter = float(rng.choice([0.0, 0.3, 0.9]))          # (0.9: returns wander into neighbouring pixels and collide)
        dirs = m.centre(u + rng.uniform(-jitter, jitter, u.shape), v + rng.uniform(-jitter, jitter, v.shape)).reshape(-1, 3)
        # a smooth surface between 0.3 and 1.6 max_ray, with noise
        r = max_ray * (0.95 + 0.65 * np.sin(u * rng.uniform(0.05, 0.4) + rng.uniform(0, 6)) * np.cos(v * rng.uniform(0.05, 0.4)))
        r = np.abs(r + rng.normal(0, 0.01, r.shape)).reshape(-1) + 0.05
        pts = (dirs * r[:, None]).astype(F)
        pts = pts[rng.random(len(pts)) > 0.08]                 # holes
        pts = pts[rng.permutation(len(pts))]
        n_dup = max(1, len(pts) // 10)
        dup = pts[rng.integers(0, len(pts), n_dup)]             # planted equal ranges: the same point again
        zr = rng.uniform(0.3, 2.0, 6)
        seam = np.stack([-zr, rng.choice([0.0, -0.0, 1e-7, -1e-7, 1e-3, -1e-3], 6), zr * np.tan(rng.uniform(min(e0, e1), max(e0, e1), 6))], 1)
        junk = np.array([[0, 0, 0], [0, 0, 1], [0, 0, -2], [-0.0, 0.0, -0.0]])
        pts = np.concatenate([pts, dup, seam.astype(F), junk.astype(F)]).astype(F)
        pts = pts[rng.permutation(len(pts))]
        rgba = rng.integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)
        dq = np.concatenate([[1.0], rng.normal(0, 0.05 * k, 3)])
        qk = np.array([q[0] * dq[0] - q[1:] @ dq[1:], *(q[0] * dq[1:] + dq[0] * q[1:] + np.cross(q[1:], dq[1:]))])
        T = np.concatenate([qk / np.linalg.norm(qk), t + rng.normal(0, 0.1 * k, 3)]).astype(F)
        scans.append((T, pts, rgba))
    return m, scans, cfg, vs, vps


def on_device(a):
    """the array in device memory -> (tensor that owns it, address)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return d, d.data_ptr()


def same_image(got, want):
    """(range, rgba [h][w][4], index) of RangeImage.download() against a restated Image -> what differs, or None"""
    rng, rgba, idx = got
    if not np.array_equal(rng.view(np.uint32), want.range.view(np.uint32)):
        return "range"
    if not np.array_equal(np.ascontiguousarray(rgba).view(np.uint32)[..., 0], want.rgba):
        return "rgba"
    if not np.array_equal(idx, want.index):
        return "point_index"
    return None


def build(capi, ctx, image, model, pts, rgba, through_scan, count=True):
    """the image from a decoded scan or from device arrays -> the build's counts"""
    if through_scan:
        data, layout = S.message(pts, rgba)
        scan = capi.Scan(ctx)
        try:
            scan.decode_msg(capi.scan_layout(**layout), data)
            return image.build(model.capi(capi), scan, count)        # (the scan may go as soon as the build is queued)
        finally:
            scan.destroy()
    (kp, pp), (kc, pc) = on_device(pts), on_device(rgba)
    out = image.build_device(model.capi(capi), pp, pc, len(pts), count)
    if not count:
        image.stats()                                                   # (the arrays are read until the build has run)
    return out


def run(capi, ctx, seed):
    """one scene on the device against the restatement -> (what differed or None, the frames' counts)"""
    m, scans, cfg, vs, vps = scene(seed)
    ref = R.Layer(vs, vps)
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, cfg.capi(capi), layer)
    image = capi.RangeImage(ctx)
    bad, all_counts = None, []
    try:
        for k, (T, pts, rgba) in enumerate(scans):
            want_img = R.build(m, pts, rgba)
            want = R.integrate(ref, T, want_img, cfg).counts
            got_img = build(capi, ctx, image, m, pts, rgba, (seed + k) % 2 == 0)
            if not R.same_counts(got_img, want_img.counts):
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
    print(f"fuzz_range_image: seeds {first}..{first + n - 1}, {n} scenes of two scans, {len(failed)} differ; totals {totals}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
