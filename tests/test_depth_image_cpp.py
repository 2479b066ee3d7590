"""GpuDepthImageIntegrator (voxgraph_amd/cpp/gpu_depth_image_integrator.h) from plain C++ over stand-in messages
(tests/cpp/image_standin.h): the header compiles and its encoding resolution runs on the CPU; on the GPU the layer
tests/cpp/depth_image_smoke.cpp builds from raw depth frames, and the counters it reads, equal the Python path's bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import depth_image_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "depth_image_smoke.cpp")
F = np.float32
DEPTH_NAMES = {D.DEPTH_16UC1: "16UC1", D.DEPTH_32FC1: "32FC1"}
COLOR_NAMES = {D.COLOR_RGB8: "rgb8", D.COLOR_BGR8: "bgr8", D.COLOR_RGBA8: "rgba8", D.COLOR_BGRA8: "bgra8", D.COLOR_MONO8: "mono8"}


def _build(tmp_path):
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libvoxgraph_amd.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "depth_image_smoke")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC,
                           "-o", exe, "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_depth_image_integrator_header_compiles_and_resolves_encodings(tmp_path):
    """no device: the three depth and five colour encodings, step / is_bigendian / K into the two structures, and the
    refusals -- other encodings, a colour image of another size"""
    r = subprocess.run([_build(tmp_path), "encodings"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "DEPTH_IMAGE_ENCODINGS_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def _pose(k):
    return D.T_ROOM_OPTICAL + F(0.04 * k) * np.array([0, 0, 0, 0, 1, -1, 0.5], F)


def _image(f, width, height, step, encoding, data):
    f.write(struct.pack("<5I", width, height, step, 0, len(encoding)) + encoding.encode() + struct.pack("<Q", len(data)))
    np.ascontiguousarray(data).tofile(f)


@pytest.mark.gpu
def test_layer_from_cpp_equals_the_python_path(tmp_path):
    from voxgraph_amd import capi
    exe = _build(tmp_path)
    vs, vps = 0.2, 16
    gate = dict(depth_unit_m=0.001, min_depth_m=3.2, max_depth_m=6.0, stride_u=2, stride_v=1)     # (the floor's near part is out)
    # a 16UC1 frame with RGB8, a 32FC1 frame with BGRA8, a "mono16" frame without colours, one with MONO8, an empty frame
    frames = [(D.room_frame(160, 120, D.DEPTH_16UC1, 0, D.COLOR_RGB8), "16UC1"), (D.room_frame(160, 120, D.DEPTH_32FC1, 1, D.COLOR_BGRA8), "32FC1"),
              (D.room_frame(97, 61, D.DEPTH_16UC1, 2, D.COLOR_NONE, row_pad=3), "mono16"), (D.room_frame(64, 48, D.DEPTH_32FC1, 3, D.COLOR_MONO8), "32FC1"),
              ((D.planted_image(0, 0, D.DEPTH_16UC1, 0), D.camera_for(0, 0)), "16UC1")]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<iif3f2i", len(frames), vps, vs, gate["depth_unit_m"], gate["min_depth_m"], gate["max_depth_m"],
                            gate["stride_u"], gate["stride_v"]))
        for k, ((img, cam), name) in enumerate(frames):
            _pose(k).tofile(f)
            np.array([cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1], np.float64).tofile(f)
            _image(f, img.width, img.height, img.row_step, name, img.depth)
            f.write(struct.pack("<I", int(img.color_kind != D.COLOR_NONE)))
            if img.color_kind != D.COLOR_NONE:
                _image(f, img.width, img.height, img.color_row_step, COLOR_NAMES[img.color_kind], img.color)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEPTH_IMAGE_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)

    ctx = capi.Context(0)
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), layer)
    scan = capi.Scan(ctx)
    counts = []
    for k, ((img, cam), _) in enumerate(frames):
        for key, v in gate.items():
            setattr(cam, key, v)
        want = D.decode(img, cam)
        got = scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color)
        assert got == (len(want[0]), D.dropped(want[3]))
        counts.append(list(got) + list(scan.depth_stats()))
        integ.integrate_scan(_pose(k), scan, count=False)
    bi, d, w, rgba = layer.download()
    assert counts[4] == [0] * 6 and all(c[0] > 1000 and c[3] > 50 and c[4] > 50 for c in counts[:4])
    raw = open(dst, "rb").read()
    nb = struct.unpack_from("<i", raw)[0]
    assert nb == len(bi) > 5
    at = 4
    for want in (bi, d, w, rgba):
        got = np.frombuffer(raw, np.uint8, want.nbytes, at)
        assert np.array_equal(got, want.reshape(-1).view(np.uint8))
        at += want.nbytes
    assert np.frombuffer(raw, np.int64, 6 * len(frames), at).reshape(-1, 6).tolist() == counts and at + 48 * len(frames) == len(raw)
    for h in (scan, integ, layer):
        h.destroy()
    ctx.close()
