"""voxgraph's three mesh markers from plain C++ (voxgraph_amd/cpp/gpu_mesh_marker.h) over the stand-in cblox / voxblox
headers and a stand-in visualization_msgs/Marker (tests/cpp/marker_standin.h): the header compiles and instantiates on
the CPU; on the GPU what tests/cpp/mesh_marker_smoke.cpp puts into the markers equals the numpy restatement
(tests/mesh_marker_ref.py) over the Python path's meshes byte for byte, with the fixed fields as stated."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_marker_ref as R
from tests.test_mesh_cpp import _submaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mesh_marker_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "mesh_marker_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims"), "-I", os.path.join(ROOT, "tests", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_mesh_marker_header_compiles_and_instantiates(tmp_path):
    """no device: the composites and DownloadMarker instantiate on the stand-in types; the mode and type values"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MESH_MARKER_COMPILE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def _read_marker(raw, at):
    n = struct.unpack_from("<q", raw, at)[0]
    mtype, locked, ns_len = struct.unpack_from("<3i", raw, at + 8)
    at += 20
    ns = raw[at:at + ns_len].decode()
    at += ns_len
    nums = struct.unpack_from("<7d", raw, at)
    alpha = struct.unpack_from("<f", raw, at + 56)[0]
    at += 60
    points = np.frombuffer(raw, np.float64, 3 * n, at).reshape(n, 3)
    at += 24 * n
    colors = np.frombuffer(raw, F, 4 * n, at).reshape(n, 4)
    return (mtype, locked, ns, nums, alpha, points, colors), at + 16 * n


@pytest.mark.gpu
def test_markers_from_cpp_equal_the_restatement(tmp_path):
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
    assert r.returncode == 0 and "MESH_MARKER_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = open(dst, "rb").read()

    ctx = capi.Context(0)
    handles = [capi.Submap(ctx, sid, vs, vps, bi, d, w) for sid, T, bi, d, w in subs]
    poses = np.stack([T for _, T, _, _, _ in subs])
    ids = [sid for sid, _, _, _, _ in subs]
    layer = capi.TsdfLayer(ctx, vs, vps)
    mesh = capi.Mesh(ctx)
    first_id = min(ids)
    at = 0
    for which, mode, opacity in (("combined", R.NORMALS, 0.5), ("separated", R.LAMBERT_COLOR, 0.75), ("submap", R.LAMBERT_COLOR, 1.0)):
        const = None
        if which == "combined":
            capi.combined_mesh(ctx, handles, poses, layer, mesh=mesh, min_weight=mw)
        elif which == "separated":
            capi.separated_mesh(ctx, handles, poses, mesh=mesh, min_weight=mw)
        else:
            handles[ids.index(first_id)].generate_mesh(mesh, mw)
            const = capi.submap_color(first_id)
        _, _, v, n = mesh.download()
        colors = mesh.download_colors() if mesh.has_colors() else None
        want = R.fill_marker(v, n, colors, mode, opacity, const)
        (mtype, locked, ns, nums, alpha, points, cols), at = _read_marker(raw, at)
        assert (mtype, locked, ns) == (R.TRIANGLE_LIST, 1, "mesh"), which
        assert nums == (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0) and alpha == float(F(opacity)), which
        assert len(points) == 3 * len(v) > 1500, which
        assert R.same(points, want[0]) and R.same(cols, want[1]), which
        if which == "separated":
            assert len(np.unique(colors, axis=0)) == len(subs)
    assert at == len(raw)
    mesh.destroy()
    layer.destroy()
    for h in handles:
        h.destroy()
    ctx.close()
