"""GenerateSeparatedMeshOnGpu + DownloadColoredMeshLayer (voxgraph_amd/cpp/gpu_mesh.h) from plain C++ against the stand-in
cblox / voxblox headers: it compiles on the CPU; on the GPU the MeshLayer it fills equals the Python path's
(capi.separated_mesh) bit for bit, colours included, with the submaps in ID order."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_mesh_cpp import _submaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "separated_mesh_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "separated_mesh_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_separated_mesh_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _read(path):
    raw = np.fromfile(path, np.uint8)
    nb = int(raw[:4].view(np.int32)[0])
    at = 4
    out = []
    for _ in range(nb):
        head = raw[at:at + 16].view(np.int32)
        nv = int(head[3])
        at += 16
        v = raw[at:at + 12 * nv].view(F).reshape(nv, 3)
        n = raw[at + 12 * nv:at + 24 * nv].view(F).reshape(nv, 3)
        c = raw[at + 24 * nv:at + 28 * nv].reshape(nv, 4)
        idx = raw[at + 28 * nv:at + 32 * nv].view(np.int32)
        at += 32 * nv
        out.append((tuple(int(x) for x in head[:3]), v, n, c, idx))
    assert at == len(raw)
    return out


@pytest.mark.gpu
def test_separated_mesh_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vps, vs, subs = _submaps()
    mw = 1e-4
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        np.array([len(subs), vps], np.int32).tofile(f)
        np.array([vs, mw], F).tofile(f)
        for sid, T, bi, d, w in subs:
            np.array([sid, len(bi)], np.int32).tofile(f)
            T.tofile(f)
            bi.tofile(f)
            d.tofile(f)
            w.tofile(f)
    outs = [tmp_path / "default.bin", tmp_path / "custom.bin"]
    r = subprocess.run([exe, str(src), *map(str, outs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SEPARATED_MESH_SMOKE_OK" in r.stdout, r.stdout + r.stderr

    ctx = capi.Context(0)
    handles = [capi.Submap(ctx, sid, vs, vps, bi, d, w) for sid, T, bi, d, w in subs]
    poses = np.stack([T for _, T, _, _, _ in subs])
    ids = [sid for sid, _, _, _, _ in subs]
    rank = {sid: k for k, sid in enumerate(sorted(ids))}
    custom = np.array([[10 * rank[i], 255 - rank[i], 7, 200] for i in ids], np.uint8)   # (per submap, in file order)
    mesh = capi.Mesh(ctx)
    for path, colors in zip(outs, (None, custom)):
        cpp = _read(path)
        capi.separated_mesh(ctx, handles, poses, colors, mesh=mesh, min_weight=mw)
        bi, first, v, n = mesh.download()
        c = mesh.download_colors()
        assert len(cpp) == len(bi) > 10 and first[-1] > 500
        for k, (idx, cv, cn, cc, ci) in enumerate(cpp):
            assert idx == tuple(int(x) for x in bi[k])
            gv = v[first[k]:first[k + 1]].reshape(-1, 3)
            gn = np.repeat(n[first[k]:first[k + 1]], 3, 0)
            gc = np.repeat(c[first[k]:first[k + 1]], 3, 0)
            assert np.array_equal(cv.view(np.uint32), gv.view(np.uint32)), idx
            assert np.array_equal(cn.view(np.uint32), gn.view(np.uint32)), idx
            assert np.array_equal(cc, gc), idx
            assert np.array_equal(ci, np.arange(len(gv))), idx
        assert len(np.unique(c, axis=0)) == len(subs)
    assert np.array_equal(np.unique(c, axis=0), np.unique(custom, axis=0))
    mesh.destroy()
    for h in handles:
        h.destroy()
    ctx.close()
