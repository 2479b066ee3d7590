"""GpuScanLocalizer (voxgraph_amd/cpp/gpu_scan_localizer.h) from plain C++: it compiles, the map config's defaults and the
hypothesis grid hold and a NULL handle is refused on the CPU; on the GPU what tests/cpp/scan_localization_smoke.cpp scores
and localises on the asymmetric room equals the Python path's byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import scan_localization_ref as R
from tests import scan_localization_scenes as S
from tests import scan_registration_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scan_localization_smoke.cpp")
F = np.float32


def _build(tmp_path):
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libvoxgraph_amd.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "scan_localization_smoke")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_localizer_compiles_and_has_the_stated_defaults(tmp_path):
    """no device: layer ESDF, no loss, stride 1; the registration config's defaults; a 3 x 1 x 4 grid; NULL handles refused"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_LOCALIZATION_COMPILE_OK 1 1 1 1 1 1" in r.stdout, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_localizer_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    sm, pts = S.room_submap(), S.scan_to_localize()
    n_yaw, stride = 12, 4                                       # (half the yaws of the full grid: 2304 hypotheses)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([sm.vps, len(sm.block_index), stride, n_yaw], np.int32).tofile(f)
        np.array([sm.voxel_size, S.MAX_ABS_DISTANCE], F).tofile(f)
        np.array([S.GRID_X[0], S.GRID_X[-1], S.GRID_Y[0], S.GRID_Y[-1], 0.5, S.GRID_Z], np.float64).tofile(f)
        np.ascontiguousarray(sm.block_index, np.int32).tofile(f)
        for a in (sm.tsdf_distance, sm.tsdf_weight, sm.esdf_distance):
            np.ascontiguousarray(a, F).tofile(f)
        np.ascontiguousarray(sm.esdf_observed, np.uint8).tofile(f)
        np.array([len(pts)], np.int64).tofile(f)
        pts.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_LOCALIZATION_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    n_poses = int(np.frombuffer(raw, np.int32, 1)[0])
    rec = np.dtype([("poses", F, (n_poses, 7)), ("best", np.int32), ("usable", np.int32), ("T", F, 7), ("delta", np.float64, 4),
                    ("cost", np.float64, n_poses), ("n_terms", np.int64, n_poses)])
    assert len(raw) == 4 + rec.itemsize
    got = np.frombuffer(raw, rec, 1, 4)[0]
    # the mirror's grid is the restatement's (as values: the mirror's zeros may be negative)
    assert np.array_equal(got["poses"], R.hypothesis_grid(S.GRID_X, S.GRID_Y, n_yaw, S.GRID_Z))

    ctx = capi.Context(0)
    submap = capi.Submap(ctx, 0, sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance, sm.tsdf_weight, sm.esdf_distance,
                         sm.esdf_observed)
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(S.MAX_ABS_DISTANCE))
    reg.set_map([submap], [[1, 0, 0, 0, 0, 0, 0]], capi.scan_map_config(score_point_stride=stride))
    reg.set_points(pts)
    cost, n_terms, _, _ = reg.score_poses(got["poses"])
    best, T, usable, delta, _ = reg.localize(got["poses"])
    assert np.array_equal(cost.view(np.uint64), got["cost"].view(np.uint64)) and np.array_equal(n_terms, got["n_terms"])
    assert best == got["best"] >= 0 and usable and got["usable"] == 1
    assert np.array_equal(got["T"].view(np.uint32), T.view(np.uint32))
    assert np.array_equal(got["delta"].view(np.uint64), delta.view(np.uint64))
    err = SR.pose_error(T, S.TRUE_POSE)
    assert err[0] < 0.5 * SR.VOXEL_SIZE and err[1] < np.radians(0.5)
    for x in (reg, submap):
        x.destroy()
    ctx.close()
