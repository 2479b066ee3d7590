"""GpuEsdfMap / GpuTsdfMap (voxgraph_amd/cpp/gpu_esdf_map.h) from plain C++: the header compiles on the CPU; on the GPU
the batch forms equal the Python path (capi.Submap.query) bit for bit, and the caller's values survive every invalid
query (tests/cpp/map_query_smoke.cpp checks that and writes its outputs)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_query_smoke.cpp")
F = np.float32
SENTINEL, GRAD_SENTINEL = 12345.5, -777.25


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "map_query_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
           "-I", os.path.join(ROOT, "oracle", "ref_shims")]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *inc, SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_query_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_map_query_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    rng = np.random.default_rng(7)
    vps, vs = 8, 0.1
    bi = synth.dense_block_index((-2, -2, -1), (4, 4, 2))
    bi = bi[rng.permutation(len(bi))][: len(bi) - 4].astype(np.int32)
    nb, nv = len(bi), vps ** 3
    td = rng.uniform(-0.3, 0.3, (nb, nv)).astype(F)
    tw = np.where(rng.random((nb, nv)) < 0.03, F(0), rng.uniform(0.1, 5, (nb, nv)).astype(F)).astype(F)
    ed = rng.uniform(-1, 2, (nb, nv)).astype(F)
    eo = (rng.random((nb, nv)) < 0.97).astype(np.uint8)
    n = 20000
    pos = rng.uniform((-1.8, -1.8, -0.9), (1.8, 1.8, 0.9), (n, 3))   # f64, some outside the map
    pos[:10] = np.nan
    T = np.array([np.cos(0.2), 0, 0, np.sin(0.2), 0.1, -0.2, 0.05], F)
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        np.array([vps, nb], np.int32).tofile(f)
        np.array([vs], F).tofile(f)
        for a in (bi, td, tw, ed, eo):
            a.tofile(f)
        np.array([n], np.int64).tofile(f)
        pos.tofile(f)
        T.tofile(f)
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MAP_QUERY_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    ctx = capi.Context(0)
    sm = capi.Submap(ctx, 0, vs, vps, bi, td, tw, ed, eo)
    p32 = pos.astype(F)   # the header's one cast

    def same(cpp_d, cpp_obs, got, sentinel):
        ok = got.valid
        assert np.array_equal(cpp_obs.astype(bool), ok) and 0 < ok.mean() < 1
        assert np.array_equal(cpp_d[ok], got.distance[ok].astype(np.float64))
        assert (cpp_d[~ok] == sentinel).all()

    for pose in (None, T):
        d, g, obs = take(np.float64, n), take(np.float64, 3 * n).reshape(n, 3), take(np.int32, n)
        got = sm.query(p32, "esdf", interpolate=True, gradient=True, pose=pose)
        same(d, obs, got, SENTINEL)
        assert np.array_equal(g[got.valid], got.gradient[got.valid].astype(np.float64))
        assert (g[~got.valid] == GRAD_SENTINEL).all()
    d, obs = take(np.float64, n), take(np.int32, n)
    same(d, obs, sm.query(p32, "tsdf", interpolate=False), SENTINEL)
    w, obs = take(np.float64, n), take(np.int32, n)
    got = sm.query(p32, "tsdf", interpolate=True, weight=True)
    assert np.array_equal(obs.astype(bool), got.valid)
    assert np.array_equal(w[got.valid], got.weight[got.valid].astype(np.float64)) and (w[~got.valid] == SENTINEL).all()
    obs = take(np.int32, n)
    assert np.array_equal(obs.astype(bool), sm.query(p32, "esdf", interpolate=False).valid)
    assert at == len(raw)
    sm.destroy()
    ctx.close()
