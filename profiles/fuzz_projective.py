"""Fuzz of projective depth-image integration (vgx_tsdf_integrate_depth_image, voxgraph_amd/csrc/vgx_projective.hip)
against its numpy restatement (tests/projective_ref.py): random cameras, poses, configurations and images, two frames
from nearby poses into one layer (so that blocks the layer already holds are met), host and device form in turn.  Every
scene is compared bit for bit: distance, weight, colour, block index in slot order and all five counts.

    python profiles/fuzz_projective.py [first_seed [n_scenes]]        (needs the GPU; profiles/fuzz_projective.txt)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import projective_ref as P  # noqa: E402

F = np.float32


def _unit_quaternion(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def scene(seed):
    """-> (frames [(pose, Image, Camera)], Config, voxel size, vps): needs no device"""
    rng = np.random.default_rng(seed)
    width, height = int(rng.integers(1, 65)), int(rng.integers(1, 49))
    vps = int(rng.choice([8, 16]))
    vs = float(rng.choice([0.05, 0.1, 0.2])) if vps == 8 else float(rng.choice([0.05, 0.1]))
    f = rng.uniform(0.6, 1.6) * max(width, height)
    cam = P.Camera(f, f * rng.uniform(0.9, 1.1), width * rng.uniform(0.3, 0.7), height * rng.uniform(0.3, 0.7),
                   depth_unit_m=float(rng.choice([0.001, 0.0005, 0.002])))
    if rng.random() < 0.5:
        cam.min_depth_m, cam.max_depth_m = float(rng.uniform(0.0, 0.8)), float(rng.uniform(1.5, 5.0))
    max_ray = float(rng.uniform(1.5, 4.0))
    cfg = P.Config(default_truncation_distance=float(vs * rng.uniform(1.5, 4.0)), max_weight=float(rng.choice([2.5, 10000.0])),
                   voxel_carving_enabled=int(rng.random() < 0.7), min_ray_length_m=float(rng.uniform(0.0, 0.7)),
                   max_ray_length_m=max_ray, use_const_weight=int(rng.random() < 0.4), allow_clear=int(rng.random() < 0.7),
                   use_weight_dropoff=int(rng.random() < 0.7))
    encoding = int(rng.choice([P.DEPTH_16UC1, P.DEPTH_32FC1]))
    kind = int(rng.integers(0, 6))
    q = _unit_quaternion(rng)
    t = rng.uniform(-1, 1, 3) * float(rng.choice([1.0, 30.0, 400.0]))
    frames = []
    for k in range(2):
        # a smooth surface between 0.3 and 1.6 max_ray with steps, noise and holes
        u, v = np.meshgrid(np.arange(width), np.arange(height))
        z = max_ray * (0.95 + 0.65 * np.sin(u * rng.uniform(0.05, 0.4) + rng.uniform(0, 6)) * np.cos(v * rng.uniform(0.05, 0.4)))
        z += rng.normal(0, 0.01, z.shape)
        z = np.abs(z) + 0.05
        bpp, pad = P.DEPTH_BPP[encoding], int(rng.choice([0, 0, 3, 8]))
        step = width * bpp + pad
        buf = rng.integers(0, 256, (height, step), dtype=np.uint8)
        hole = rng.random(z.shape) < 0.08
        if encoding == P.DEPTH_16UC1:
            px = np.round(z / cam.depth_unit_m).clip(0, 65535).astype("<u2")
            px[hole] = 0
        else:
            px = z.astype("<f4")
            px[hole] = rng.choice(np.array([np.nan, 0.0, -0.0, -1.0, np.inf, -np.inf], "<f4"), int(hole.sum()))
        buf[:, :width * bpp] = px.view(np.uint8).reshape(height, width * bpp)
        cbpp = P.COLOR_BPP[kind]
        cstep = width * cbpp + int(rng.choice([0, 1, 5]))
        color = rng.integers(0, 256, height * cstep, dtype=np.uint8) if cbpp else None
        img = P.Image(width, height, encoding, buf, step, kind, color, cstep if cbpp else None)
        dq = np.concatenate([[1.0], rng.normal(0, 0.05 * k, 3)])
        qk = np.array([q[0] * dq[0] - q[1:] @ dq[1:], *(q[0] * dq[1:] + dq[0] * q[1:] + np.cross(q[1:], dq[1:]))])
        T = np.concatenate([qk / np.linalg.norm(qk), t + rng.normal(0, 0.1 * k, 3)]).astype(F)
        frames.append((T, img, cam))
    return frames, cfg, vs, vps


def same_layer(got, want):
    """bit for bit: block index, distance, weight, rgba -> the name of the first array that differs, or None"""
    for name, g, w in zip(("block_index", "distance", "weight", "rgba"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.shape != w.shape or not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            return name
    return None


def on_device(a, shift):
    """the bytes of `a` in device memory `shift` bytes past a multiple of 256 -> (tensor that owns them, address)"""
    import torch
    d = torch.zeros(len(a) + 16, dtype=torch.uint8, device="cuda")
    d[shift:shift + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d, d.data_ptr() + shift


def run(capi, ctx, seed):
    """one scene on the device against the restatement -> (what differed or None, the frames' counts)"""
    frames, cfg, vs, vps = scene(seed)
    ref = P.Layer(vs, vps)
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, cfg.capi(capi), layer)
    bad, all_counts = None, []
    try:
        for k, (T, img, cam) in enumerate(frames):
            want = P.integrate(ref, T, img, cam, cfg).counts
            if (seed + k) % 2 == 0:
                got = integ.integrate_depth_image(T, img.layout(capi), cam.capi(capi), img.depth, img.color)
            else:
                shift = int(seed % 3)
                (kd, pd) = on_device(img.depth, shift)
                (kc, pc) = on_device(img.color, shift) if img.color is not None else (None, None)
                got = integ.integrate_depth_image_device(T, img.layout(capi), cam.capi(capi), pd, len(img.depth), pc,
                                                         0 if img.color is None else len(img.color))
            all_counts.append(got)
            if got != want:
                bad = bad or f"frame {k}: counts {got} != {want}"
        bad = bad or same_layer(layer.download(), ref.download())
    finally:
        integ.destroy()
        layer.destroy()
    return bad, all_counts


def main():
    from voxgraph_amd import capi
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
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
    print(f"fuzz_projective: seeds {first}..{first + n - 1}, {n} scenes of two frames, {len(failed)} differ; totals {totals}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
