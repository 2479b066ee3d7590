"""The undistorting path of GpuPointcloudIntegrator and GpuScanTrack (voxgraph_amd/cpp/gpu_pointcloud_integrator.h) from
plain C++: timeFieldOf over stand-in messages and its refusals on the CPU; on the GPU the scan
tests/cpp/scan_undistort_smoke.cpp decodes, its counters and the knots GpuScanTrack forms equal the Python path's bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import scan_undistort_ref as U
from tests import scan_undistort_scenes as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scan_undistort_smoke.cpp")
F = np.float32


def _build(tmp_path):
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libvoxgraph_amd.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "scan_undistort_smoke")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC,
                           "-o", exe, "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_time_field_detection_and_its_refusals(tmp_path):
    """no device: t (UINT32) before time (FLOAT32) before timestamp (FLOAT64), each with count 1, whatever the order of
    the fields; a message without any of them is refused; the host-only check takes what the mirror makes"""
    r = subprocess.run([_build(tmp_path), "fields"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_UNDISTORT_FIELDS_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def _samples(n):
    """odometry in a fixed frame: a sensor turning about a tilted axis while it moves, quaternions not quite of unit length"""
    t = 1000.0 + np.linspace(0.0, 0.11, n) ** 1.1
    ang = 0.4 + 1.0 * (t - t[0])
    axis = np.array([0.1, -0.2, 0.97])
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], 1) * 1.001
    pos = np.stack([5.0 + 2.0 * (t - t[0]), -3.0 + 0.3 * np.sin(20 * t), 1.0 + 0.05 * np.cos(9 * t)], 1)
    return t, np.concatenate([q, pos], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["driver48", "step27_f64_at19"])
def test_mirror_from_cpp_equals_the_python_path(tmp_path, name):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    stamp = 1000.0 if name == "driver48" else Z.STAMP                   # (the f64 layout's times are absolute)
    m, f, _ = Z.message(name, 1031, 5, seed=6, row_pad=3)
    t, poses = _samples(40)
    t = t - 1000.0 + stamp
    ref = poses[-1]
    Ts = np.array([np.cos(0.1), 0, 0, np.sin(0.1), 0.3, -0.2, 0.1], F)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<6I", m.width, m.height, m.point_step, m.row_step, m.is_bigendian, len(m.fields)))
        for fname, offset, datatype, count in m.fields:
            fh.write(struct.pack("<I", len(fname)) + fname.encode() + struct.pack("<3I", offset, datatype, count))
        fh.write(struct.pack("<Q", len(m.data)))
        np.ascontiguousarray(m.data).tofile(fh)
        fh.write(struct.pack("<d", stamp))
        ref.astype(np.float64).tofile(fh)
        Ts.tofile(fh)
        fh.write(struct.pack("<i", len(t)))
        np.concatenate([t[:, None], poses], 1).astype(np.float64).tofile(fh)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_UNDISTORT_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)

    track = capi.ScanTrack()
    for tk, Tk in zip(t, poses):
        track.add(tk, Tk)
    kt, kT = track.relative_to(ref, stamp)
    ctx = capi.Context(0)
    scan = capi.Scan(ctx)
    field = capi.scan_time_field(f.kind, f.offset, f.scale, -stamp if f.kind == U.TIME_FLOAT64 else 0.0)
    n, dropped = scan.decode_undistorted(m.layout(capi), m.data, field, kt, kT)
    pts, rgba = scan.download()
    ustats = scan.undistort_stats()
    assert 0 < n < m.n and ustats[2] > 0 and np.abs(kT[0, 4:]).max() > 0.1
    raw = open(dst, "rb").read()
    assert struct.unpack_from("<i", raw)[0] == len(kt) == 40
    at = 4
    for want in (kt, kT, np.array([n, dropped, *ustats], np.int64), pts, rgba):
        got = np.frombuffer(raw, np.uint8, want.nbytes, at)
        assert np.array_equal(got, np.ascontiguousarray(want).reshape(-1).view(np.uint8))
        at += want.nbytes
    assert struct.unpack_from("<i", raw, at)[0] > 5 and at + 4 == len(raw)
    # and the Python path is the restatement's
    want = U.decode(m, U.TimeField(f.kind, f.offset, f.scale, field.offset_s), kt, kT)
    assert np.array_equal(pts.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(rgba, want[1])
    scan.destroy()
    ctx.close()
