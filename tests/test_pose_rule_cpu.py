"""The one pose rule (voxgraph_amd/csrc/vgx_pose.h) without a GPU: tests/cpp/pose_rule_check.cpp includes that header alone,
is built with AddressSanitizer and UBSan as a program of its own and prints bit patterns; here every line is recomputed --
the rotations, the rigid transforms and the inverses with tests/projected_map_ref.py under exact equality of the f32
words, pose_defect's verdicts with the stated rule (all seven values finite, else | |q|^2 - 1 | <= 1e-4 in f64)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import projected_map_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")                                         # the compiler the library's own Makefile names
    assert cxx is not None
    exe = str(tmp_path_factory.mktemp("pose_rule") / "pose_rule_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "voxgraph_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pose_rule_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stderr)
    assert out.returncode == 0 and "pose_rule_check ok" in out.stdout and "ERROR" not in out.stderr
    return out.stdout.splitlines()


def words(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint32)


def test_rotation_rigid_transform_and_inverse_match_the_restatement_bit_for_bit(lines):
    rows = [words(l.split()[1:]) for l in lines if l.startswith("R ")]
    assert len(rows) > 400
    for w in rows:
        f = w.view(F)
        q, t, v = f[0:4], f[4:7], f[7:10]
        rot, rig, qi, ti = w[10:13], w[13:16], w[16:20], w[20:23]
        assert np.array_equal(ref.quat_rotate(q, v.reshape(1, 3))[0].view(np.uint32), rot)
        assert np.array_equal(ref.transform(q, t, v.reshape(1, 3))[0].view(np.uint32), rig)
        rqi, rti = ref.inverse(np.concatenate([q, t]))
        assert np.array_equal(rqi.view(np.uint32), qi)
        # the library forms -(q^-1 t + 0), the restatement -(q^-1 t): the same word unless q^-1 t has a component -0
        assert np.array_equal(rti.view(np.uint32), ti)
    # the table holds large and small rotations and both signs of every quaternion component
    qs = np.array([w.view(F)[0:4] for w in rows])
    assert (qs > 0.5).any(0).all() and (qs < -0.5).any(0).all()


def stated_rule(T):
    if not np.isfinite(T).all():
        return 1
    d = T[:4].astype(np.float64)
    n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]
    return 2 if abs(n2 - 1.0) > 1e-4 else 0


def test_pose_defect_follows_the_stated_rule(lines):
    rows = [l.split() for l in lines if l.startswith("D ")]
    seen = set()
    near = {(-1, 0): 0, (-1, 2): 0, (1, 0): 0, (1, 2): 0}   # (side of 1, verdict) among the nearly-unit poses
    for r in rows:
        T = words(r[1:8]).view(F)
        verdict = int(r[8])
        assert verdict == stated_rule(T), (T, verdict)
        seen.add(verdict)
        if np.isfinite(T).all():
            d = T[:4].astype(np.float64)
            n2 = float((d * d).sum())
            if 5e-5 < abs(n2 - 1.0) < 2e-4:
                near[(1 if n2 > 1.0 else -1, verdict)] += 1
    assert seen == {0, 1, 2}
    assert all(c > 0 for c in near.values()), near                   # both bounds are approached from both sides
    # not finite wins over not unit
    both = [r for r in rows if not np.isfinite(words(r[1:8]).view(F)).all() and (words(r[1:5]).view(F) == 2.0).any()]
    assert both and all(int(r[8]) == 1 for r in both)
