"""voxgraph's map publishers and voxblox's deserializeMsgToLayer from plain C++ (voxgraph_amd/cpp/gpu_map_messages.h) over
stand-in messages (tests/cpp/map_msgs_standin.h): the header compiles and instantiates on the CPU; on the GPU what
tests/cpp/map_msg_smoke.cpp puts into the messages equals the numpy restatement (tests/map_msg_ref.py) bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import map_msg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_msg_smoke.cpp")
F = np.float32


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "map_msg_smoke")
    lib = os.path.join(ROOT, "voxgraph_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voxgraph_amd", "cpp"), "-I", os.path.join(ROOT, "tests", "cpp"), SRC,
                           "-o", exe, "-L", lib, "-lvoxgraph_amd", "-lpthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_messages_header_compiles_and_instantiates(tmp_path):
    """no device: every publisher instantiates on the stand-in types, T_B_S of two hand-worked poses, the action values"""
    r = subprocess.run([_build(tmp_path), "compile"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MAP_MSG_COMPILE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)


def _read_layer_msg(raw, at):
    n, action, esdf, vps = struct.unpack_from("<4I", raw, at)
    vs = struct.unpack_from("<d", raw, at + 16)[0]
    at += 24
    bi = np.frombuffer(raw, np.int32, 3 * n, at).reshape(n, 3)
    at += 12 * n
    per = vps ** 3 * (2 if esdf else 3)
    words = np.frombuffer(raw, np.uint32, n * per, at).reshape(n, per)
    return (action, esdf, vps, vs, bi, words), at + 4 * n * per


@pytest.mark.gpu
def test_messages_from_cpp_equal_the_restatement(tmp_path):
    exe = _build(tmp_path)
    rng = np.random.default_rng(11)
    vps, vs, nb, npts = 8, 0.1, 7, 333
    nv = vps ** 3
    bi = np.ascontiguousarray(rng.permutation(np.stack(np.meshgrid(range(40, 43), range(-46, -43), range(2), indexing="ij"), -1)
                                              .reshape(-1, 3))[:nb], np.int32)
    d = rng.uniform(-0.4, 0.4, (nb, nv)).astype(F)
    w = np.where(rng.random((nb, nv)) < 0.2, F(0), rng.uniform(0, 9, (nb, nv)).astype(F)).astype(F)
    d[0, :4] = [np.nan, np.inf, -0.0, -np.inf]
    rgba = rng.integers(0, 256, (nb, nv, 4), dtype=np.uint8)
    rgba[0, 0] = [1, 2, 3, 4]
    ed = rng.uniform(-2, 2, (nb, nv)).astype(F)
    eo = (rng.random((nb, nv)) < 0.6).astype(np.uint8)
    eo[0, :2] = [200, 0]
    yaw, pose = 0.4, None
    pose = np.array([np.cos(yaw / 2), 0.02, -0.03, np.sin(yaw / 2), 1.5, -0.7, 0.3], np.float64)
    pose[:4] /= np.linalg.norm(pose[:4])
    pose = pose.astype(F)
    xyz = rng.uniform(-3, 3, (npts, 3)).astype(F)
    pw = rng.uniform(0, 50, npts).astype(F)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<iiif", vps, nb, npts, vs))
        for a in (pose, bi, d, w, rgba, ed, eo, xyz, pw):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MAP_MSG_SMOKE_OK" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = open(dst, "rb").read()
    # 1. the projected-map message: kReset, the layer's words with colours
    (action, esdf, mvps, mvs, mbi, words), at = _read_layer_msg(raw, 0)
    assert (action, esdf, mvps, mvs) == (R.RESET, 0, vps, float(F(vs)))
    assert R.same(mbi, bi) and R.same(words, R.tsdf_words(d, w, rgba))
    # 2. the layer deserialised from it (into a layer that held something else)
    nr = struct.unpack_from("<i", raw, at)[0]
    at += 4
    assert nr == nb
    got = []
    for dtype, count in ((np.int32, 3 * nr), (F, nr * nv), (F, nr * nv), (np.uint8, 4 * nr * nv)):
        got.append(np.frombuffer(raw, dtype, count, at))
        at += got[-1].nbytes
    have = R.as_dict(got[0].reshape(nr, 3), got[1].reshape(nr, nv), got[2].reshape(nr, nv), got[3].reshape(nr, nv, 4))
    assert R.same_layers(have, R.as_dict(bi, d, w, rgba))
    # 3. the submap messages: TSDF without colours, ESDF with observed as 0 / 1
    for want_esdf, want in ((0, R.tsdf_words(d, w)), (0, R.tsdf_words(d, w)), (1, R.esdf_words(ed, eo))):
        (action, esdf, mvps, mvs, mbi, words), at = _read_layer_msg(raw, at)
        assert (action, esdf, mvps) == (R.RESET, want_esdf, vps) and R.same(mbi, bi) and R.same(words, want)
    # 4. the surface cloud, as it is and moved by T_B_S = T_S_B.inverse()
    T = np.frombuffer(raw, F, 12, at).reshape(3, 4)
    at += 48
    qw, qx, qy, qz = pose[:4].astype(np.float64)
    Rm = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                   [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                   [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    assert np.abs(T[:, :3] - Rm.T).max() < 1e-6 and np.abs(T[:, 3] + Rm.T @ pose[4:].astype(np.float64)).max() < 1e-6
    for t in (None, T):
        data = np.frombuffer(raw, np.uint8, 32 * npts, at).reshape(npts, 32)
        at += 32 * npts
        assert R.same(data, R.surface_bytes(xyz, pw, t))
    assert at == len(raw)
