"""GpuScanToMapRegisterer (voxgraph_amd/cpp/gpu_scan_to_map_registerer.h) from plain C++: every overload compiles and the
config's defaults hold on the CPU; on the GPU the poses tests/cpp/scan_registration_smoke.cpp refines equal the Python
path's byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import scan_registration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scan_registration_smoke.cpp")
F = np.float32


def _build(tmp_path):
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libvoxgraph_amd.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "scan_registration_smoke")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_registerer_compiles_and_has_the_stated_defaults(tmp_path):
    """no device: min_range 0, max_range +inf, stride 1, ratio 0.5, no default distance, a NULL context refused"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_REGISTRATION_COMPILE_OK 1 1 1 1 1 1" in r.stdout, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_registerer_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    scans = [(R.pose7(R.scan_pose(k)), R.room_scan(R.scan_pose(k))) for k in range(6)]
    pts = R.room_scan(R.scan_pose(6))
    priors = np.stack([R.pose7(R.seeded_prior(s)) for s in (0, 3, 5)])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([len(scans), R.VPS, len(priors)], np.int32).tofile(f)
        np.array([R.VOXEL_SIZE, R.MAX_ABS_DISTANCE], F).tofile(f)
        for T, p in scans:
            T.tofile(f)
            np.array([len(p)], np.int64).tofile(f)
            p.tofile(f)
        np.array([len(pts)], np.int64).tofile(f)
        pts.tofile(f)
        priors.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCAN_REGISTRATION_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    rec = np.dtype([("usable", np.int32), ("T", F, 7), ("delta", np.float64, 4)])
    got = np.fromfile(dst, rec)
    assert len(got) == len(priors)

    ctx = capi.Context(0)
    layer = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS)
    integrator = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for T, p in scans:
        integrator.integratePointCloud(T, p)
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE))
    reg.set_points(pts)
    for k, prior in enumerate(priors):
        T, usable, delta, _ = reg.refine(layer, prior)
        assert usable and got["usable"][k] == 1
        assert np.array_equal(got["T"][k].view(np.uint32), T.view(np.uint32)), k
        assert np.array_equal(got["delta"][k].view(np.uint64), delta.view(np.uint64)), k
        assert not np.array_equal(T.view(np.uint32), prior.view(np.uint32))
    for x in (reg, integrator, layer):
        x.destroy()
    ctx.close()
