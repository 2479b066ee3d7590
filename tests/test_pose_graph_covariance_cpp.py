"""voxgraph_amd/cpp/gpu_pose_graph.h's edge covariances from plain C++ (tests/cpp/pose_graph_covariance_smoke.cpp): the
header compiles under -Wall -Wextra -Werror and the two 6x6 fill helpers are exact without a device; on the GPU
GpuPoseGraph::getEdgeCovarianceMap on the solved 8-submap ring gives the blocks the Python wrapper gives on the same
nodes and edges (to rounding: the sqrt-information comes from two 4x4 factorisations, as tests/test_pose_graph_cpp.py
explains), and false for an unknown id."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_graph_covariance_smoke.cpp")


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "pose_graph_covariance_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_covariance_header_compiles_and_the_fill_helpers_are_exact(tmp_path):
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "POSE_GRAPH_COVARIANCE_COMPILE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def ring_of_8(capi):
    """the graph of tests/cpp/pose_graph_smoke.cpp: node 0 the reference frame, nodes 1..8 the submaps 100..107"""
    n, pi = 8, math.pi
    poses = np.zeros((n + 1, 4))
    for k in range(n):
        a = 2.0 * pi * k / n
        poses[k + 1] = [2.0 * math.cos(a) - 2.0 + 0.05 * k, 2.0 * math.sin(a) - 0.03 * k, 0.01 * k, 0.9 * a / pi - 0.01 * k]
    odo = np.diag(np.sqrt([1.0, 1.0, 2500.0, 2500.0]))
    loop = np.linalg.cholesky(np.array([[100.0, 20, 0, 0], [20, 100, 0, 0], [0, 0, 2500, 0], [0, 0, 0, 2500]])).T
    edges = []
    for k in range(n - 1):
        a, b = 2.0 * pi * k / n, 2.0 * pi * (k + 1) / n
        dx, dy, ya = 2.0 * (math.cos(b) - math.cos(a)), 2.0 * (math.sin(b) - math.sin(a)), 0.9 * a / pi
        t = [math.cos(ya) * dx + math.sin(ya) * dy, -math.sin(ya) * dx + math.cos(ya) * dy, 0.0]
        edges.append(capi.pose_graph_edge(k + 1, k + 2, t, 0.9 * (b - a) / pi, odo))
    a = 2.0 * pi * (n - 1) / n
    ya, dx, dy = 0.9 * a / pi, 2.0 * (1.0 - math.cos(a)), -2.0 * math.sin(a)
    edges.append(capi.pose_graph_edge(n, 1, [math.cos(ya) * dx + math.sin(ya) * dy, -math.sin(ya) * dx + math.cos(ya) * dy, 0.0], -ya, loop))
    edges.append(capi.pose_graph_edge(0, 1 + n // 2, [-4.0, 0.0, 0.0], 0.9, odo))
    return poses, edges, [1, 1] + [0] * (n - 1)


@pytest.mark.gpu
def test_cpp_edge_covariance_map_is_the_python_wrappers(tmp_path):
    from voxgraph_amd import capi
    dst = tmp_path / "out.bin"
    r = subprocess.run([_build(tmp_path), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "POSE_GRAPH_COVARIANCE_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
    got = np.fromfile(dst, np.float64)
    poses, edges, constant = ring_of_8(capi)
    ctx = capi.Context(0)
    pg = capi.PoseGraph(ctx, 9, constant)
    pg.set_edges(edges)
    x, s = pg.optimize(poses)
    # the map's order: keys sorted; submap id 100 + k is node 1 + k
    ids = sorted([(101, 102), (102, 101), (103, 107), (100, 104), (105, 105), (107, 101)])
    blocks = pg.covariance(x, [(a - 99, b - 99) for a, b in ids])
    pg.destroy()
    ctx.close()
    assert len(got) == 32 + 16 * len(ids)
    np.testing.assert_allclose(got[:32].reshape(8, 4), x[1:], rtol=0, atol=1e-10)
    theirs = got[32:].reshape(len(ids), 4, 4)
    print("max |block|", np.abs(blocks).max(), "max difference", np.abs(theirs - blocks).max())
    assert not theirs[0].any() and not blocks[0].any()                   # (100, 104): submap 100 is constant
    assert all(np.abs(b).max() > 0 for b in theirs[1:])
    np.testing.assert_allclose(theirs, blocks, rtol=1e-10, atol=1e-10)
