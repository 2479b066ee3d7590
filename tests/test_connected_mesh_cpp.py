"""ConnectMeshOnGpu + DownloadConnectedMesh (voxgraph_amd/cpp/gpu_mesh.h) from plain C++ against the stand-in cblox /
voxblox headers: it compiles on the CPU; on the GPU the Mesh it fills equals the Python path's (capi.Mesh.connect) bit
for bit, for the collection's separated mesh (with colours) and its combined mesh (without), through one reused handle."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_mesh_cpp import _submaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "connected_mesh_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "connected_mesh_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_connected_mesh_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _read(path):
    raw = np.fromfile(path, np.uint8)
    nv, nt, has = (int(x) for x in raw[:24].view(np.int64))
    at = 24
    v = raw[at:at + 12 * nv].view(F).reshape(nv, 3)
    n = raw[at + 12 * nv:at + 24 * nv].view(F).reshape(nv, 3)
    at += 24 * nv
    c = raw[at:at + 4 * nv].reshape(nv, 4) if has else None
    at += 4 * nv if has else 0
    idx = raw[at:at + 12 * nt].view(np.uint32).reshape(nt, 3)
    assert at + 12 * nt == len(raw)
    return v, n, c, idx


@pytest.mark.gpu
def test_connected_mesh_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vps, vs, subs = _submaps()
    mw = 1e-4
    thresholds = np.array([1e-10, 0.5 * vs], F)
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        np.array([len(subs), vps], np.int32).tofile(f)
        np.array([vs, mw], F).tofile(f)
        thresholds.tofile(f)
        for sid, T, bi, d, w in subs:
            np.array([sid, len(bi)], np.int32).tofile(f)
            T.tofile(f)
            bi.tofile(f)
            d.tofile(f)
            w.tofile(f)
    outs = [tmp_path / "separated.bin", tmp_path / "combined.bin"]
    r = subprocess.run([exe, str(src), *map(str, outs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONNECTED_MESH_SMOKE_OK" in r.stdout, r.stdout + r.stderr

    ctx = capi.Context(0)
    handles = [capi.Submap(ctx, sid, vs, vps, bi, d, w) for sid, T, bi, d, w in subs]
    poses = np.stack([T for _, T, _, _, _ in subs])
    mesh = capi.Mesh(ctx)
    layer = capi.TsdfLayer(ctx, vs, vps)
    out = capi.ConnectedMesh(ctx)
    for k, path in enumerate(outs):
        if k == 0:
            capi.separated_mesh(ctx, handles, poses, mesh=mesh, min_weight=mw)
        else:
            capi.combined_mesh(ctx, handles, poses, layer, mesh, mw)
        want = mesh.connect(thresholds[k], out).download()
        got = _read(path)
        assert len(want[3]) > 500 and len(want[0]) <= 0.5 * 3 * len(want[3])
        assert (want[2] is not None) == (k == 0)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    for o in [out, mesh, layer] + handles:
        o.destroy()
    ctx.close()
