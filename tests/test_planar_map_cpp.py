"""The planar map from plain C++ (voxgraph_amd/cpp/gpu_planar_map.h) with the OccupancyGrid stand-in of
tests/cpp/occupancy_grid_standin.h: it compiles on the CPU; on the GPU every grid of tests/cpp/planar_map_smoke.cpp equals
the Python path's byte for byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "planar_map_smoke.cpp")
F = np.float32


def _build(tmp_path):
    exe = str(tmp_path / "planar_map_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")          # (tests/conftest.py has built it where it was missing)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC, "-o", exe,
                           "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_planar_map_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def _read_maps(path, n_maps):
    raw = open(path, "rb").read()
    at, out = 0, []
    for _ in range(n_maps):
        res = np.frombuffer(raw, F, 1, at)[0]
        w, h = (int(v) for v in np.frombuffer(raw, np.uint32, 2, at + 4))
        origin = np.frombuffer(raw, np.float64, 3, at + 12)
        counts = tuple(int(v) for v in np.frombuffer(raw, np.int64, 3, at + 36))
        at += 60
        data = np.frombuffer(raw, np.int8, w * h, at).reshape(h, w)
        at += w * h
        fields = []
        for _ in range(3):
            fields.append(np.frombuffer(raw, F, w * h, at).reshape(h, w))
            at += 4 * w * h
        out.append((res, (w, h), origin, counts, data, *fields))
    assert at == len(raw)
    return out


@pytest.mark.gpu
def test_grids_from_cpp_equal_the_python_path(tmp_path):
    from tests import planar_map_ref as R
    from tests import planar_map_scenes as S
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    sc = S.SCENES["band_vps8"]()
    cfg = dict(sc.configs[2], unknown_is_obstacle=1, min_free_voxels=2)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([sc.vps, len(sc.bi)], np.int32).tofile(f)
        np.array([sc.voxel_size], F).tofile(f)
        f.write(bytes(capi.planar_map_config(**cfg)))
        for a in (sc.bi, sc.d, sc.w, sc.d, sc.o):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PLANAR_MAP_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    maps = _read_maps(dst, 3)

    ctx = capi.Context(0)
    sm = capi.Submap(ctx, 0, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    layer = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
    layer.upload(sc.bi, sc.d, sc.w)
    pm = capi.PlanarMap(ctx)
    c = capi.planar_map_config(**cfg)
    for got, run in zip(maps, (lambda: layer.planar_map(c, pm), lambda: sm.layer_planar_map("tsdf", c, pm),
                               lambda: sm.layer_planar_map("esdf", c, pm))):
        run()
        (x0, y0), dim, vs, counts = pm.stats()
        state, occ, clear, height, dist = pm.download()
        res, gdim, origin, gcounts, data, gdist, gclear, gheight = got
        assert min(counts) > 0 and gdim == dim and gcounts == counts and res == F(vs)
        assert origin.tolist() == [float(F(x0) * F(vs)), float(F(y0) * F(vs)), 0.5 * (float(F(cfg["z_min"])) + float(F(cfg["z_max"])))]
        assert R.same(data, occ) and R.same(gdist, dist) and R.same(gclear, clear) and R.same(gheight, height)
    for h in (pm, layer, sm):
        h.destroy()
    ctx.close()
