"""voxgraph_amd/cpp/gpu_pose_graph.h's edge covariances on the tile-sparse factor from plain C++
(tests/cpp/pose_graph_sparse_covariance_smoke.cpp): the header compiles under -Wall -Wextra -Werror; on the GPU
GpuPoseGraph::getEdgeCovarianceMap with the tile-sparse solver gives, on a ring whose every input is a literal, the very
bytes the Python wrapper gives at the poses the C++ solve ended at; and the map succeeds on a chain of 4200 submaps,
which the dense solver refuses."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_graph_sparse_covariance_smoke.cpp")


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "pose_graph_sparse_covariance_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sparse_covariance_header_compiles(tmp_path):
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "POSE_GRAPH_SPARSE_COVARIANCE_COMPILE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def sqrt_information(information):
    """voxgraph_amd::SqrtInformation operation by operation (scalar f64, the same order): L^T of the LLT of a 4x4 matrix"""
    A = [[float(v) for v in row] for row in information]
    L = [[0.0] * 4 for _ in range(4)]
    for j in range(4):
        d = A[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 4):
            v = A[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    return np.array(L).T.copy()


def literal_ring(capi):
    """the graph of the smoke's ring(): node 0 the reference frame, nodes 1..8 the submaps 100..107"""
    odo = sqrt_information(np.diag([1.0, 1.0, 2500.0, 2500.0]))
    loop = sqrt_information([[100.0, 20, 0, 0], [20, 100, 0, 0], [0, 0, 2500, 0], [0, 0, 0, 2500]])
    edges = [capi.pose_graph_edge(k + 1, k + 2, [1.0, 0.25 * (k % 3) - 0.25, 0.01], 0.1, odo) for k in range(7)]
    edges.append(capi.pose_graph_edge(8, 1, [0.5, -1.0, -0.07], -0.7, loop))
    edges.append(capi.pose_graph_edge(0, 5, [2.0, 2.0, 0.04], 0.4, odo))
    return edges, [1, 1] + [0] * 7


@pytest.mark.gpu
def test_cpp_edge_covariance_map_on_the_sparse_factor_is_the_python_wrappers_bytes(tmp_path):
    from voxgraph_amd import capi
    dst = tmp_path / "out.bin"
    r = subprocess.run([_build(tmp_path), str(dst)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "POSE_GRAPH_SPARSE_COVARIANCE_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
    got = np.fromfile(dst, np.float64)
    ids = sorted([(101, 102), (102, 101), (103, 107), (100, 104), (105, 105), (107, 101)])  # the map's order
    assert len(got) == 32 + 16 * len(ids)
    poses = np.zeros((9, 4))
    poses[1:] = got[:32].reshape(8, 4)                                   # where the C++ solve ended; node 0 is the frame
    edges, constant = literal_ring(capi)
    ctx = capi.Context(0)
    pg = capi.PoseGraph(ctx, 9, constant, linear_solver=capi.LINEAR_SOLVER_TILE_SPARSE, ordering=capi.ORDER_RCM)
    pg.set_edges(edges)
    blocks, stats = pg.covariance_sparse(poses, [(a - 99, b - 99) for a, b in ids])
    pg.destroy()
    ctx.close()
    theirs = got[32:].reshape(len(ids), 4, 4)
    print(stats, "max |block|", np.abs(blocks).max(), "max difference", np.abs(theirs - blocks).max())
    assert stats["n_columns"] == 16 and not theirs[0].any()              # (100, 104): submap 100 is constant
    assert all(np.abs(b).max() > 0 for b in theirs[1:])
    assert theirs.tobytes() == blocks.tobytes()
