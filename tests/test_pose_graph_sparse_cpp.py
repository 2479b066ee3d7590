"""GpuPoseGraph::setLinearSolver from plain C++ (tests/cpp/pose_graph_sparse_smoke.cpp): the header compiles and refuses a
bad permutation without a device; on the GPU the tile-sparse solver in natural order ends at the dense solver's poses
value for value, and under RCM within 1e-6 of them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_graph_sparse_smoke.cpp")


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "pose_graph_sparse_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sparse_pose_graph_header_compiles_and_refuses_a_bad_permutation(tmp_path):
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "POSE_GRAPH_SPARSE_COMPILE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_cpp_sparse_graph_ends_where_the_dense_one_ends(tmp_path):
    r = subprocess.run([_build(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "POSE_GRAPH_SPARSE_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
