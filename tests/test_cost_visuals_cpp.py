"""The cost-function visuals from plain C++ (voxgraph_amd/cpp/gpu_registration_cost_function.h with
gpu_cost_function_visuals.h) over the Ceres stub and the stand-in visualization_msgs/Marker: the headers compile and
instantiate on the CPU; on the GPU what tests/cpp/cost_visuals_smoke.cpp's recording sink receives equals the Python
path byte for byte, with the marker constants and T_mission__reading as stated."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import synth
from tests import cost_visuals_ref as R
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cost_visuals_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "cost_visuals_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "tests", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cost_visuals_headers_compile_and_instantiate(tmp_path):
    """no device: the Config defaults, the marker constants, FillJacobianMarkers on the stand-in, the host transform"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "COST_VISUALS_COMPILE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


class _Reader:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.raw, self.at)
        self.at += struct.calcsize("<" + fmt)
        return v

    def string(self):
        (n,) = self.take("i")
        s = self.raw[self.at:self.at + n].decode()
        self.at += n
        return s

    def array(self, dtype, count):
        a = np.frombuffer(self.raw, dtype, count, self.at)
        self.at += a.nbytes
        return a

    def marker(self):
        frame, ns = self.string(), self.string()
        head = self.take("4i")
        nums = self.take("7d")
        rgba = self.take("4f")
        (n,) = self.take("q")
        return dict(frame=frame, ns=ns, id=head[0], type=head[1], action=head[2], frame_locked=head[3], scale=nums[:3],
                    orientation=nums[3:], color=rgba, points=self.array(np.float64, 3 * n).reshape(n, 3))


def _check_marker(m, want, points):
    assert (m["frame"], m["ns"], m["id"], m["type"], m["action"], m["frame_locked"]) == \
        (R.FRAME, want["ns"], want["id"], want["type"], 0, 0)
    assert m["scale"] == want["scale"] and m["orientation"] == (0.0, 0.0, 0.0, 1.0) and m["color"] == want["color"]
    assert R.same(m["points"], points), want["ns"]


@pytest.mark.gpu
def test_sink_receives_what_the_python_path_computes(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    sm, _ = synth.config1_pair()
    xyz, dist, _ = H.oracle_points(sm)
    n = 2 * 1024 + 4
    step = len(xyz) // n
    xyz, dist = np.ascontiguousarray(xyz[::step][:n]), np.ascontiguousarray(dist[::step][:n])
    w = np.where(np.arange(n) % 2 == 0, F(0.25), F(0.75)).astype(F)
    ref_pose, read_pose = np.array([0.31, -0.22, 0.05, 3.1]), np.array([0.36, -0.16, 0.32, -3.12])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([sm.vps, sm.n_blocks, n], np.int32).tofile(f)
        np.array([sm.voxel_size], F).tofile(f)
        for a in (sm.block_index.astype(np.int32), sm.tsdf_distance, sm.tsdf_weight, sm.esdf_distance, sm.esdf_observed,
                  xyz, dist, w, ref_pose, read_pose):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "COST_VISUALS_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
    rd = _Reader(open(dst, "rb").read())

    ctx = capi.Context(0)
    g = H.gpu_submap(capi, ctx, sm)
    g.set_points(capi.POINTS_VOXELS, xyz, dist, w)
    cf = capi.RegistrationCostFunction(ctx, g, g, capi.default_config(registration_point_type=capi.POINTS_VOXELS))
    vis = capi.RegVisuals(ctx)
    q, t = R.mission_pose(read_pose)
    for with_jac in (True, False):
        rows = np.zeros(n)
        jo, je = (np.zeros((n, 4)), np.zeros((n, 4))) if with_jac else (None, None)
        assert cf.evaluate_visuals([ref_pose, read_pose], rows, [jo, je] if with_jac else None, vis)
        cloud, arrows, origins, _ = vis.download()
        assert rd.take("4i") == (1, 1, 1, 1 if with_jac else 0)
        assert R.same(rd.array(F, 4), q) and R.same(rd.array(F, 3), t)
        assert (rd.string(), rd.string()) == (R.FRAME, R.CHILD_FRAME)
        assert rd.take("4I") == (n, 1, R.POINT_STEP, R.POINT_STEP * n) and rd.string() == R.FRAME
        assert R.same(rd.array(np.uint8, 32 * n).reshape(n, 32), cloud)
        if with_jac:
            assert len(origins) == n
            _check_marker(rd.marker(), R.ARROWS, arrows)
            _check_marker(rd.marker(), R.ORIGINS, origins)
        assert R.same(rd.array(np.float64, n), rows)
        if with_jac:
            assert R.same(rd.array(np.float64, 4 * n).reshape(n, 4), je)
    # the flags false: the same rows, and the sink was never called
    assert rd.take("4i") == (1, 0, 0, 0)
    assert R.same(rd.array(np.float64, n), rows)
    rd.array(np.float64, 4 * n)
    assert rd.at == len(rd.raw)
    vis.destroy()
    cf.destroy()
    g.destroy()
    ctx.close()
