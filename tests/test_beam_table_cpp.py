"""GpuPointcloudIntegrator::integrateProjective for a beam table and sortedBeamTable
(voxgraph_amd/cpp/gpu_pointcloud_integrator.h) from plain C++ over a stand-in message (tests/cpp/pointcloud2_standin.h): the
overload compiles, the helper sorts a table in laser order and the host-only calls answer on the CPU; on the GPU the layer
the method builds from one sweep (counted, then queued) equals the one the C ABI builds, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "beam_table_smoke.cpp")


def _build(tmp_path):
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libvoxgraph_amd.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "beam_table_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC,
                           "-o", exe, "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_beam_overload_compiles_the_table_is_sorted_and_the_host_only_calls_answer(tmp_path):
    r = subprocess.run([_build(tmp_path), "header"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "BEAM_TABLE_HEADER_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_layer_from_the_beam_overload_equals_the_c_abi(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BEAM_TABLE_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
