"""The layer point clouds from plain C++ (voxgraph_amd/cpp/gpu_layer_pointcloud.h, and GpuMapEvaluation's error-cloud
arguments in gpu_map_evaluation.h) against the stand-in headers of oracle/ref_shims: they compile on the CPU; on the GPU
every cloud of tests/cpp/layer_cloud_smoke.cpp equals the Python path's bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "layer_cloud_smoke.cpp")
F = np.float32


def _inc():
    return ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"),
            "-I", os.path.join(ROOT, "oracle", "ref_shims")]


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "layer_cloud_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", *_inc(), SRC, "-o", exe, "-L", lib, "-lvoxgraph_amd",
                           "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_layer_pointcloud_header_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


def test_map_evaluation_header_with_the_error_cloud_compiles(tmp_path):
    src = tmp_path / "eval_cloud.cpp"
    src.write_text('#include "gpu_map_evaluation.h"\n#include "gpu_layer_pointcloud.h"\n'
                   "template <class CollectionT>\n"
                   "vgx_voxel_evaluation_details run(const voxgraph_amd::GpuMapEvaluation& e, const CollectionT& c, voxgraph_amd::GpuCloud* cloud,\n"
                   "                                 float voxel_size) {\n"
                   "  const vgx_cloud_config cfg = voxgraph_amd::LayerCloudConfig(VGX_CLOUD_DISTANCE, 0.6, 2, 3 * voxel_size);\n"
                   "  return e.evaluate(c, nullptr, &cfg, cloud->handle()).details;\n}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", *_inc(), "-I", os.path.join(ROOT, "tests", "stubs"),
                           str(src)])


def _read_clouds(path, n_clouds):
    raw = open(path, "rb").read()
    at, out = 0, []
    for _ in range(n_clouds):
        n = int(np.frombuffer(raw, np.int64, 1, at)[0])
        out.append(np.frombuffer(raw, np.uint8, 16 * n, at + 8).reshape(n, 16))
        at += 8 + 16 * n
    return out, raw[at:]


def _packed(cloud, colour=False):
    xyz, inten, rgba = cloud.download()
    rec = np.zeros((len(xyz), 16), np.uint8)
    rec[:, :12] = xyz.view(np.uint8).reshape(-1, 12)
    rec[:, 12:] = (rgba if colour else inten.view(np.uint8).reshape(-1, 4))
    return rec


@pytest.mark.gpu
def test_clouds_from_cpp_equal_the_python_path(tmp_path):
    from tests import layer_cloud_scenes as S
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    sc = S.SCENES["random_vps8"]()
    rng = np.random.default_rng(4)
    keep = rng.permutation(len(sc.bi))[:45]                      # the test side: most of the blocks, in another order
    bi2 = np.ascontiguousarray(sc.bi[keep])
    ed2 = (sc.d[keep] + rng.normal(0, 0.01, sc.d[keep].shape)).astype(F)
    eo2 = np.ascontiguousarray(sc.o[keep])
    sd, axis = F(0.6), 2
    plane = F(next(c["slice_value"] for c in sc.configs if c.get("slice_axis") == axis))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([sc.vps, len(sc.bi)], np.int32).tofile(f)
        np.array([sc.voxel_size, sd, plane], F).tofile(f)
        np.array([axis], np.int32).tofile(f)
        for a in (sc.bi, sc.d, sc.w, sc.d, sc.o, sc.rgba):
            np.ascontiguousarray(a).tofile(f)
        np.array([len(bi2)], np.int32).tofile(f)
        for a in (bi2, ed2, eo2):
            a.tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LAYER_CLOUD_SMOKE_OK" in r.stdout, r.stdout + r.stderr
    clouds, tail = _read_clouds(dst, 9)

    ctx = capi.Context(0)
    sm = capi.Submap(ctx, 0, sc.voxel_size, sc.vps, sc.bi, sc.d, sc.w, sc.d, sc.o)
    test = capi.Submap(ctx, 1, sc.voxel_size, sc.vps, bi2, ed2, ed2, ed2, eo2)
    layer = capi.TsdfLayer(ctx, sc.voxel_size, sc.vps)
    layer.upload(sc.bi, sc.d, sc.w, sc.rgba)
    cloud = capi.Cloud(ctx)
    cc = capi.cloud_config
    sliced = dict(slice_axis=axis, slice_value=float(plane))
    want = [_packed(layer.cloud(cc(), cloud)),
            _packed(layer.cloud(cc(kind=capi.CLOUD_SURFACE_DISTANCE, surface_distance=sd), cloud)),
            _packed(layer.cloud(cc(kind=capi.CLOUD_SURFACE_COLOR, surface_distance=sd), cloud), colour=True),
            _packed(layer.cloud(cc(**sliced), cloud)),
            _packed(sm.layer_cloud("tsdf", cc(kind=capi.CLOUD_SURFACE_DISTANCE, surface_distance=sd), cloud)),
            _packed(sm.layer_cloud("esdf", cc(), cloud)),
            _packed(sm.layer_cloud("esdf", cc(**sliced), cloud))]
    details = []
    for cfg in (cc(), cc(**sliced)):
        det, _ = capi.evaluate_layers_rmse_cloud(sm, test, capi.EVAL_LAYER_ESDF, capi.EVAL_IGNORE_BEHIND_TEST, cfg, cloud)
        want.append(_packed(cloud))
        details.append(det)
    for k, (got, exp) in enumerate(zip(clouds, want)):
        assert 0 < len(exp) < sc.d.size and got.shape == exp.shape and np.array_equal(got, exp), k
    size = C.sizeof(capi.EvaluationDetails)
    assert len(tail) == 2 * size
    for k, det in enumerate(details):
        got = capi.EvaluationDetails.from_buffer_copy(tail[k * size:(k + 1) * size]).as_dict()
        assert set(got) == set(det) and det["num_evaluated_voxels"] > 1000
        for key in det:                                # as bytes: the scene plants NaN distances, so the sum is NaN
            assert np.float64(got[key]).tobytes() == np.float64(det[key]).tobytes(), (key, got[key], det[key])
    for h in (cloud, layer, test, sm):
        h.destroy()
    ctx.close()
