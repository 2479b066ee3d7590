"""GpuViewRenderer (voxgraph_amd/cpp/gpu_view_renderer.h) from plain C++: every overload compiles and the config's defaults
and ray helpers hold on the CPU; on the GPU the view tests/cpp/view_render_smoke.cpp renders, the pose it registers from
the view's points and the layer it integrates them into equal the Python path's byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import scan_registration_ref as R
from tests import view_render_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "view_render_smoke.cpp")
F = np.float32
CFG = dict(s_max=12.0, min_step=0.05, unknown_step=0.2, max_bracket=0.65)
MIN_RANGE = 0.05


def _build(tmp_path):
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libvoxgraph_amd.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "view_render_smoke")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_renderer_compiles_and_has_the_stated_defaults(tmp_path):
    """no device: s_min 0, step_scale 0.75, image_width 0, flags = points; the four fields without a default are zero and
    refused; unit rays; a NULL context refused"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VIEW_RENDER_COMPILE_OK 1 1 1 1 1 1" in r.stdout, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_renderer_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    scans = [(R.pose7(R.scan_pose(k)), R.room_scan(R.scan_pose(k))) for k in range(6)]
    T_view, dirs, prior = R.pose7(R.scan_pose(6)), V.room_dirs(), R.pose7(R.seeded_prior(3))
    n = len(dirs)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([len(scans), R.VPS, 256], np.int32).tofile(f)
        np.array([R.VOXEL_SIZE, R.MAX_ABS_DISTANCE, MIN_RANGE], F).tofile(f)
        np.array([0.0, CFG["s_max"], 0.75, CFG["min_step"], CFG["unknown_step"], CFG["max_bracket"]], F).tofile(f)
        for T, p in scans:
            T.tofile(f)
            np.array([len(p)], np.int64).tofile(f)
            p.tofile(f)
        T_view.tofile(f)
        np.array([n], np.int64).tofile(f)
        dirs.tofile(f)
        prior.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VIEW_RENDER_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    rec = np.dtype([("counts", np.int64, 8), ("range", F, n), ("status", np.uint8, n), ("points", F, (n, 3)), ("gradient", F, (n, 3)),
                    ("weight", F, n), ("rgba", np.uint8, (n, 4)), ("n_samples", np.int32, n), ("usable", np.int32), ("T", F, 7),
                    ("blocks", np.int32)])
    got = np.fromfile(dst, rec)
    assert len(got) == 1
    got = got[0]

    ctx = capi.Context(0)
    layer = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS)
    integrator = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    for T, p in scans:
        integrator.integratePointCloud(T, p)
    view = capi.View(ctx, capi.view_config(flags=capi.VIEW_ALL, **CFG))      # (the other ray mapping: the same bytes)
    image = layer.render_view(view, T_view, dirs).download()
    counts = view.stats()
    assert [int(c) for c in got["counts"][:7]] == [counts[k] for k in V.COUNTS] and counts["n_hit"] > 0.7 * n
    for name in capi.ViewImage._fields:
        assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint8), np.ascontiguousarray(getattr(image, name)).view(np.uint8)), name
    reg = capi.ScanRegistration(ctx, capi.scan_registration_config(R.MAX_ABS_DISTANCE, min_range_m=MIN_RANGE))
    reg.set_points(view.device_pointers().points, n)
    T, usable, _, _ = reg.refine(layer, prior)
    assert usable and got["usable"] == 1 and np.array_equal(got["T"].view(np.uint32), T.view(np.uint32))
    assert not np.array_equal(T.view(np.uint32), prior.view(np.uint32))
    second = capi.TsdfLayer(ctx, R.VOXEL_SIZE, R.VPS)
    into = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), second)
    into.integrate_device(T_view, view.device_pointers().points, None, n)
    assert got["blocks"] == second.stats()[0] > 0
    for x in (reg, view, into, second, integrator, layer):
        x.destroy()
    ctx.close()
