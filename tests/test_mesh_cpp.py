"""GenerateCombinedMeshOnGpu + DownloadMeshLayer (voxgraph_amd/cpp/gpu_mesh.h) from plain C++ against the stand-in cblox
/ voxblox headers: it compiles on the CPU; on the GPU the MeshLayer it fills equals the Python path's
(capi.combined_mesh) bit for bit, with the submaps merged in ID order."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mesh_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "mesh_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_mesh_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _submaps():
    """three overlapping submaps holding a sphere's sdf, inserted out of ID order"""
    vps, vs = 8, 0.2
    out = []
    for sid, yaw, t in ((7, 0.3, (0.2, -0.1, 0.0)), (2, -0.9, (0.5, 0.4, 0.1)), (5, 2.0, (-0.3, 0.2, -0.1))):
        bi = np.array([(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-1, 2)], np.int32)
        i = np.arange(vps ** 3)
        local = (np.stack([i % vps, (i // vps) % vps, i // (vps * vps)], -1) + 0.5) * vs
        p = bi[:, None, :] * (vps * vs) + local[None]
        d = (np.linalg.norm(p - np.array([0.1 * sid, 0.05, -0.1]), axis=-1) - 1.1).astype(F)
        w = np.full(d.shape, 1.0 + sid, F)
        T = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2), *t], F)
        out.append((sid, T, bi, d, w))
    return vps, vs, out


@pytest.mark.gpu
def test_combined_mesh_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vps, vs, subs = _submaps()
    mw = 1e-4
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([len(subs), vps], np.int32).tofile(f)
        np.array([vs, mw], F).tofile(f)
        for sid, T, bi, d, w in subs:
            np.array([sid, len(bi)], np.int32).tofile(f)
            T.tofile(f)
            bi.tofile(f)
            d.tofile(f)
            w.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESH_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint8)
    nb = int(raw[:4].view(np.int32)[0])
    at = 4
    cpp = []
    for _ in range(nb):
        head = raw[at:at + 16].view(np.int32)
        nv = int(head[3])
        at += 16
        v = raw[at:at + 12 * nv].view(F).reshape(nv, 3)
        n = raw[at + 12 * nv:at + 24 * nv].view(F).reshape(nv, 3)
        idx = raw[at + 24 * nv:at + 28 * nv].view(np.int32)
        at += 28 * nv
        cpp.append((tuple(int(c) for c in head[:3]), v, n, idx))
    assert at == len(raw)

    ctx = capi.Context(0)
    handles = [capi.Submap(ctx, sid, vs, vps, bi, d, w) for sid, T, bi, d, w in subs]
    poses = np.stack([T for _, T, _, _, _ in subs])
    layer = capi.TsdfLayer(ctx, vs, vps)
    mesh = capi.combined_mesh(ctx, handles, poses, layer, min_weight=mw)
    bi, first, v, n = mesh.download()
    assert len(cpp) == len(bi) > 10 and first[-1] > 500
    for k, (idx, cv, cn, ci) in enumerate(cpp):
        assert idx == tuple(int(c) for c in bi[k])
        gv = v[first[k]:first[k + 1]].reshape(-1, 3)
        gn = np.repeat(n[first[k]:first[k + 1]], 3, 0)
        assert np.array_equal(cv.view(np.uint32), gv.view(np.uint32)), idx
        assert np.array_equal(cn.view(np.uint32), gn.view(np.uint32)), idx
        assert np.array_equal(ci, np.arange(len(gv))), idx
    # ID order, not insertion order: merging in file order gives another layer, hence another mesh
    other = capi.TsdfLayer(ctx, vs, vps)
    other.merge_submaps(handles, poses)
    ov = other.generate_mesh().download()[2]
    assert ov.shape != v.shape or not np.array_equal(ov.view(np.uint32), v.view(np.uint32))
    mesh.destroy()
    layer.destroy()
    other.destroy()
    for h in handles:
        h.destroy()
    ctx.close()
