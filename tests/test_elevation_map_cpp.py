"""The elevation map from plain C++ (voxgraph_amd/cpp/gpu_elevation_map.h) with the GridMap stand-in of
tests/cpp/grid_map_standin.h: it compiles on the CPU; on the GPU every layer of tests/cpp/elevation_map_smoke.cpp equals
the Python path's byte for byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "elevation_map_smoke.cpp")
F = np.float32


def _build(tmp_path):
    exe = str(tmp_path / "elevation_map_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")          # (tests/conftest.py has built it where it was missing)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC, "-o", exe,
                           "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_elevation_map_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _read_maps(path, n_maps):
    raw = open(path, "rb").read()
    at, out = 0, []
    for _ in range(n_maps):
        info = np.frombuffer(raw, np.float64, 6, at)
        h, w = (int(v) for v in np.frombuffer(raw, np.uint32, 2, at + 48))
        states = tuple(int(v) for v in np.frombuffer(raw, np.int64, 4, at + 56))
        classes = tuple(int(v) for v in np.frombuffer(raw, np.int64, 3, at + 88))
        at += 112
        layers = []
        for _ in range(6):
            layers.append(np.frombuffer(raw, F, w * h, at).reshape(h, w))
            at += 4 * w * h
        out.append((info, (w, h), states, classes, layers))
    assert at == len(raw)
    return out


@pytest.mark.gpu
def test_layers_from_cpp_equal_the_python_path(tmp_path):
    from tests import elevation_map_ref as R
    from tests import elevation_map_scenes as S
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    sc = S.SCENES["tilted_vps8"]()
    cfg = dict(sc.configs[3], min_free_voxels=2)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([sc.vps, len(sc.bi)], np.int32).tofile(f)
        np.array([sc.voxel_size], F).tofile(f)
        f.write(bytes(capi.elevation_map_config(**cfg)))
        for a in (sc.bi, sc.d, sc.w, sc.d, sc.o):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ELEVATION_MAP_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    maps = _read_maps(dst, 3)

    ctx = capi.Context(0)
    sm = capi.Submap(ctx, 0, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    layer = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
    layer.upload(sc.bi, sc.d, sc.w)
    em = capi.ElevationMap(ctx)
    c = capi.elevation_map_config(**cfg)
    for got, run in zip(maps, (lambda: layer.elevation_map(c, em), lambda: sm.layer_elevation_map("tsdf", c, em),
                               lambda: sm.layer_elevation_map("esdf", c, em))):
        run()
        (x0, y0), (w, h), vs, states, classes = em.stats()
        a = dict(zip(R.FIELDS, em.download()))
        info, gdim, gstates, gclasses, layers = got
        assert min(states) > 0 and min(classes) > 0 and gdim == (w, h) and gstates == states and gclasses == classes
        vsd = float(F(vs))
        assert info.tolist() == [vsd, w * vsd, h * vsd, (x0 + 0.5 * w) * vsd, (y0 + 0.5 * h) * vsd,
                                 0.5 * (float(F(cfg["z_min"])) + float(F(cfg["z_max"])))]
        surface, nan = a["state"] == 1, F(np.nan)
        want = [np.where(surface, a["height"], nan), np.where(a["slope_valid"] != 0, a["slope"], nan), np.where(surface, a["step"], nan),
                np.where(surface, a["headroom"].astype(F) * F(vs), nan), a["cls"].astype(F), a["distance"]]
        for name, g, x in zip(("elevation", "slope", "step", "headroom", "traversability", "distance"), layers, want):
            assert R.same(g, x.astype(F)), name
    for h in (em, layer, sm):
        h.destroy()
    ctx.close()
