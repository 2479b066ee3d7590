"""The colour opt-ins of the C++ mirrors (voxgraph_amd/cpp: GpuSubmapRegistry::setKeepColors / UploadFinishedSubmap's
keep_colors, FinishSubmapOnGpu's keep_colors, GenerateCombinedMeshOnGpu's use_color, DownloadColoredMeshLayer and the
markers on a per-vertex mesh) from plain C++ over the stand-in cblox / voxblox headers: they compile and default to off on
the CPU; on the GPU what tests/cpp/map_colour_smoke.cpp writes equals the Python path byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_mesh_cpp import _submaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_colour_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "map_colour_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims"), "-I", os.path.join(ROOT, "tests", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_colour_opt_ins_compile_and_default_to_off(tmp_path):
    """no device: every mirror call instantiates without its opt-in argument; the layout constants"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MAP_COLOUR_COMPILE_OK 1 0 1 2" in r.stdout, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_colour_opt_ins_from_cpp_equal_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vps, vs, subs = _submaps()
    rng = np.random.default_rng(0)
    rgbas = [rng.integers(0, 256, d.shape + (4,), dtype=np.uint8) for _, _, _, d, _ in subs]
    mw = 1e-4
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([len(subs), vps], np.int32).tofile(f)
        np.array([vs, mw], F).tofile(f)
        for (sid, T, bi, d, w), c in zip(subs, rgbas):
            np.array([sid, len(bi)], np.int32).tofile(f)
            T.tofile(f)
            bi.tofile(f)
            d.tofile(f)
            w.tofile(f)
            c.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MAP_COLOUR_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint8)
    flags = raw[:24].view(np.int32)
    # defaults: no submap keeps colours, the mesh has none; opt-ins: all keep them, one colour per vertex;
    # FinishSubmapOnGpu: off, then on
    assert flags.tolist() == [0, capi.MESH_COLORS_NONE, len(subs), capi.MESH_COLORS_PER_VERTEX, 0, 1]
    nb = int(raw[24:28].view(np.int32)[0])
    at = 28
    cpp = []
    for _ in range(nb):
        head = raw[at:at + 16].view(np.int32)
        nv = int(head[3])
        at += 16
        v = raw[at:at + 12 * nv].view(F).reshape(nv, 3)
        c = raw[at + 12 * nv:at + 16 * nv].reshape(nv, 4)
        at += 16 * nv
        cpp.append((tuple(int(x) for x in head[:3]), v, c))
    n_points = int(raw[at:at + 8].view(np.int64)[0])
    at += 8
    marker = raw[at:at + 16 * n_points].view(F).reshape(n_points, 4)
    at += 16 * n_points
    kb = int(raw[at:at + 4].view(np.int32)[0])
    at += 4
    kept_bi = raw[at:at + 12 * kb].view(np.int32).reshape(kb, 3)
    at += 12 * kb
    kept_rgba = raw[at:at + 4 * kb * vps ** 3].reshape(kb, vps ** 3, 4)
    at += 4 * kb * vps ** 3
    assert at == len(raw)

    ctx = capi.Context(0)
    handles = [capi.Submap(ctx, sid, vs, vps, bi, d, w) for sid, T, bi, d, w in subs]
    for h, c in zip(handles, rgbas):
        h.set_colors(c)
    poses = np.stack([T for _, T, _, _, _ in subs])
    layer = capi.TsdfLayer(ctx, vs, vps)
    mesh = capi.combined_mesh(ctx, handles, poses, layer, min_weight=mw, use_color=True)
    bi, first, v, n = mesh.download()
    vc = mesh.download_vertex_colors()
    assert len(cpp) == len(bi) > 10 and first[-1] > 500
    assert len(np.unique(vc.reshape(-1, 4), axis=0)) > 100
    for k, (idx, cv, cc) in enumerate(cpp):
        assert idx == tuple(int(x) for x in bi[k])
        assert np.array_equal(cv.view(np.uint32), v[first[k]:first[k + 1]].reshape(-1, 3).view(np.uint32)), idx
        assert np.array_equal(cc, vc[first[k]:first[k + 1]].reshape(-1, 4)), idx
    m = capi.fill_marker(mesh, color_mode=capi.MARKER_LAMBERT_COLOR, opacity=0.7)
    want = m.download()[1]
    assert marker.shape == want.shape and np.array_equal(marker.view(np.uint32), want.view(np.uint32))
    # the submap finished from the projected map with keep_colors: the layer's colours in the submap's block order
    lbi, _, _, lrgba = layer.download()
    row = {tuple(int(x) for x in b): i for i, b in enumerate(lbi)}
    assert kb == len(lbi)
    assert np.array_equal(kept_rgba, lrgba[[row[tuple(int(x) for x in b)] for b in kept_bi]])
    for x in handles + [m, mesh, layer]:
        x.destroy()
    ctx.close()
