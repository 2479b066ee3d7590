"""GpuMapEvaluation (voxgraph_amd/cpp/gpu_map_evaluation.h) from plain C++ against the stand-in cblox / voxblox headers
and the Ceres stand-in: it compiles on the CPU; on the GPU its alignment agrees with the Python path's (the harness
solver) within 1 mm / 0.01 deg, and at the same aligned pose the Python path (capi.map_evaluation) gives the same details
bit for bit and the same T_ground_truth__reading.  (How close either alignment comes to the offset the ground truth was
built with is tests/test_map_eval_gpu.py's check.)"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_eval_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "map_eval_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims"), "-I", os.path.join(ROOT, "tests", "stubs")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_evaluation_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _yaw_pose(p):
    return np.array([np.cos(p[3] / 2), 0, 0, np.sin(p[3] / 2), p[0], p[1], p[2]], F)


@pytest.mark.gpu
def test_map_evaluation_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    from tests.test_map_eval_gpu import _Align, _compose4
    exe = _build(tmp_path)
    ctx = capi.Context(0)
    vs, vps = 0.1, 16
    poses = [np.array([1.6 * k, 0.3 * np.sin(k), 0.03 * k, 0.1 * k]) for k in range(3)]
    subs = [capi.Submap.synth_city(ctx, k, vs, vps, (-4, -4, -4), (8, 8, 8), 0.3, 2.0, 10.0, p, 3)
            for k, p in enumerate(poses)]
    off = np.array([-0.05, 0.03, 0.01, np.deg2rad(-1.0)])
    layer = capi.TsdfLayer(ctx, vs, vps)
    capi.projected_map(ctx, subs, np.stack([_yaw_pose(_compose4(off, p)) for p in poses]), layer)
    gbi, gd, gw, _ = layer.download()
    layer.destroy()
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        np.array([len(subs), vps], np.int32).tofile(f)
        np.array([vs], F).tofile(f)
        for k, (sm, p) in enumerate(zip(subs, poses)):
            td, tw, _, _ = sm.download_layers(vps)
            bi = sm.block_index()
            np.array([k, len(bi)], np.int32).tofile(f)
            _yaw_pose(p).tofile(f)
            bi.tofile(f)
            td.tofile(f)
            tw.tofile(f)
        np.array([len(gbi)], np.int32).tofile(f)
        gbi.tofile(f)
        gd.tofile(f)
        gw.tofile(f)
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "MAP_EVAL_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    m = re.search(r"POSE (\S+) (\S+) (\S+) (\S+) ITERATIONS (\d+)", r.stdout)
    cpp_pose = np.array([float(m.group(i)) for i in range(1, 5)])
    cpp_T = np.array([float(v) for v in re.search(r"T_GT_READING (.*)", r.stdout).group(1).split()])
    vals = re.search(r"DETAILS (.*)", r.stdout).group(1).split()
    cpp = [float.fromhex(v) for v in vals[:5]] + [int(v) for v in vals[5:]]

    gt = capi.Submap(ctx, 100, vs, vps, gbi, gd, gw)
    T7 = np.stack([_yaw_pose(p) for p in poses])
    align = _Align(ctx)
    py = capi.map_evaluation(ctx, subs, T7, gt, align)
    assert np.abs(py["pose4"][:3] - cpp_pose[:3]).max() < 1e-3 and abs(np.rad2deg(py["pose4"][3] - cpp_pose[3])) < 0.01
    assert np.abs(cpp_T[4:] - off[:3]).max() < 5e-3 and abs(np.rad2deg(2 * np.arctan2(cpp_T[3], cpp_T[0]) - off[3])) < 0.05
    at_cpp = capi.map_evaluation(ctx, subs, T7, gt, lambda ref, read: cpp_pose)
    d = at_cpp["details"]
    want = [d["rmse"], d["max_error"], d["min_error"], d["total_squared_error"], d["min_abs_error"],
            d["num_evaluated_voxels"], d["num_ignored_voxels"], d["num_overlapping_voxels"], d["num_non_overlapping_voxels"]]
    assert cpp == want, (cpp, want)
    assert np.allclose(at_cpp["T_ground_truth__reading"], cpp_T, rtol=0, atol=1e-12)
    for h in subs + [gt]:
        h.destroy()
    ctx.close()
