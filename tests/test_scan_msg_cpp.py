"""voxgraph::PointcloudIntegrator's mirror from plain C++ (voxgraph_amd/cpp/gpu_pointcloud_integrator.h) over stand-in
messages (tests/cpp/pointcloud2_standin.h): the header compiles and its field detection runs on the CPU; on the GPU the
layer tests/cpp/scan_msg_smoke.cpp builds from raw messages equals the Python path's bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import scan_msg_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scan_msg_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "scan_msg_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC,
                           "-o", exe, "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pointcloud_integrator_header_compiles_and_detects_fields(tmp_path):
    """no device: layoutOf over stand-in messages -- rgb wins over intensity, other fields are ignored, coordinates that
    are not one FLOAT32 and an intensity that is not FLOAT32 are refused"""
    r = subprocess.run([_build(tmp_path), "layout"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_MSG_LAYOUT_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def _pose(k):
    return np.array([np.cos(0.05 * k), 0, 0, np.sin(0.05 * k), 0.1 + 0.15 * k, -0.05 * k, 0.02], F)


@pytest.mark.gpu
def test_layer_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vs, vps = 0.2, 16
    # an XYZI LiDAR with dropped beams, an unaligned RGB cloud, a driver's 48-byte points, a cloud without colours and
    # without a dropped point (the one that keeps its width), an empty message
    whole = S.Msg(64, 16, 16, S.XYZ).fill(np.random.default_rng(3), np.random.default_rng(4).uniform(-6, 6, (1024, 3)))
    msgs = [S.lidar(30), S.small("unaligned19_rgb", 5, width=300, height=7, row_pad=3), S.lidar(31, name="driver48"), whole,
            S.Msg(0, 0, 16, S.XYZ), S.depth(32, rows=120, cols=160)]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<iiif", len(msgs), vps, 1, vs))
        for k, m in enumerate(msgs):
            _pose(k).tofile(f)
            f.write(struct.pack("<6I", m.width, m.height, m.point_step, m.row_step, m.is_bigendian, len(m.fields)))
            for name, offset, datatype, count in m.fields:
                f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<3I", offset, datatype, count))
            f.write(struct.pack("<Q", len(m.data)))
            np.ascontiguousarray(m.data).tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SCAN_MSG_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)

    ctx = capi.Context(0)
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    scan = capi.Scan(ctx)
    counts = []
    for k, m in enumerate(msgs):
        counts.append(scan.decode_msg(m.layout(capi), m.data)[0])
        integ.integrate_scan(_pose(k), scan, count=False)
    bi, d, w, rgba = layer.download()
    assert counts[3] == 1024 and counts[4] == 0 and all(0 < c < m.n for c, m in zip(counts[:3], msgs[:3]))
    raw = open(dst, "rb").read()
    nb = struct.unpack_from("<i", raw)[0]
    assert nb == len(bi) > 5
    at = 4
    for want in (bi, d, w, rgba):
        got = np.frombuffer(raw, np.uint8, want.nbytes, at)
        assert np.array_equal(got, want.reshape(-1).view(np.uint8))
        at += want.nbytes
    assert np.frombuffer(raw, np.int64, len(msgs), at).tolist() == counts and at + 12 * len(msgs) == len(raw)
    # the integrator is told the message's width only where no point was dropped: a compacted cloud is not organised
    assert np.frombuffer(raw, np.int32, len(msgs), at + 8 * len(msgs)).tolist() == [0, 0, 0, 64, 0, 0]
    for h in (scan, integ, layer):
        h.destroy()
    ctx.close()
