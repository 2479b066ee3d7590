"""GetProjectedMapOnGpu (voxgraph_amd/cpp/gpu_projected_map.h) from plain C++ against the stand-in cblox / voxblox
headers of oracle/ref_shims: it compiles on the CPU; on the GPU its voxblox layer equals the Python path's
(capi.projected_map) bit for bit, and the submaps are merged in ID order, not insertion order."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "projected_map_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "projected_map_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_projected_map_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _submaps():
    rng = np.random.default_rng(4)
    vps, vs = 8, 0.2
    out = []
    for sid, yaw, t in ((7, 0.3, (0.2, -0.1, 0.0)), (2, -0.9, (0.5, 0.4, 0.1)), (5, 2.0, (-0.3, 0.2, -0.1))):
        bi = np.array([(x, y, z) for x in range(-1, 2) for y in range(-1, 2) for z in range(0, 2)], np.int32)
        d = rng.uniform(-0.4, 0.4, (len(bi), vps ** 3)).astype(F)
        w = rng.uniform(0.5, 10, (len(bi), vps ** 3)).astype(F)
        w[rng.random(w.shape) < 0.05] = 0
        T = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)
        out.append((sid, T, bi, d, w))
    return vps, vs, out


@pytest.mark.gpu
def test_projected_map_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vps, vs, subs = _submaps()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([len(subs), vps], np.int32).tofile(f)
        np.array([vs], F).tofile(f)
        for sid, T, bi, d, w in subs:
            np.array([sid, len(bi)], np.int32).tofile(f)
            T.tofile(f)
            bi.tofile(f)
            d.tofile(f)
            w.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PROJECTED_MAP_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint8)
    nb = int(raw[:4].view(np.int32)[0])
    rec = raw[4:].reshape(nb, 12 + 8 * vps ** 3)
    cpp = {tuple(int(v) for v in r[:12].view(np.int32)): (r[12:12 + 4 * vps ** 3].view(F), r[12 + 4 * vps ** 3:].view(F))
           for r in rec}

    ctx = capi.Context(0)
    handles = [capi.Submap(ctx, sid, vs, vps, bi, d, w) for sid, T, bi, d, w in subs]
    poses = np.stack([T for _, T, _, _, _ in subs])
    results = []
    for order in ([0, 1, 2], [1, 2, 0]):       # insertion order, ID order (2, 5, 7)
        layer = capi.TsdfLayer(ctx, vs, vps)
        if order == [0, 1, 2]:
            layer.merge_submaps([handles[i] for i in order], poses[order])
        else:
            capi.projected_map(ctx, handles, poses, layer)
        bi, d, w, _ = layer.download()
        results.append({tuple(int(v) for v in b): (dd, ww) for b, dd, ww in zip(bi, d, w)})
        layer.destroy()
    insertion, by_id = results
    assert set(cpp) == set(by_id) and len(cpp) > 10
    for k in by_id:
        assert np.array_equal(cpp[k][0].view(np.uint32), by_id[k][0].view(np.uint32)), k
        assert np.array_equal(cpp[k][1].view(np.uint32), by_id[k][1].view(np.uint32)), k
    assert any(not np.array_equal(cpp[k][0], insertion[k][0]) for k in insertion)
    for h in handles:
        h.destroy()
    ctx.close()
