"""Cost-function visuals without a device: properties of the numpy restatement (tests/cost_visuals_ref.py) and the new
surface of the library and of its Python view."""
import ctypes as C
import os

import numpy as np

from oracle import pyoracle as orc
from tests import cost_visuals_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_intensity_rounding_chain():
    """(float)((double)(float)r_u * factor): narrowed BEFORE the scaling, scaled in f64, rounded once"""
    r_u = np.array([0.1234567890123, -3.3e-5, 0.0, 1.0 / 3.0, 0.25 * 0.75])
    for factor in (1.0, 2.0, 1.37, 7.0 / 3.0):
        got = R.intensity(r_u, factor)
        assert got.dtype == F
        for a, g in zip(r_u, got):
            assert g == F(np.float64(F(a)) * np.float64(factor))
    # the chain is not f32(r_u * factor): a value where narrowing first changes the result
    hits = 0
    for a in np.random.default_rng(0).uniform(-1, 1, 4000):
        hits += int(R.intensity([a], 7.0 / 3.0)[0] != F(a * (7.0 / 3.0)))
    assert hits > 0
    # ... nor an f32 product
    hits = 0
    for a in np.random.default_rng(1).uniform(-1, 1, 4000):
        hits += int(R.intensity([a], 7.0 / 3.0)[0] != F(a) * F(7.0 / 3.0))
    assert hits > 0
    # a power-of-two factor only moves the exponent
    assert R.same(R.intensity(r_u, 2.0), (r_u.astype(F) * F(2)))


def test_tip_equals_origin_for_a_zero_jacobian():
    p_m = np.random.default_rng(2).uniform(-50, 50, (33, 3)).astype(F)
    arrows, origins = R.jacobian_points(p_m, np.zeros((33, 3), F), 1.75)
    assert arrows.shape == (66, 3) and origins.shape == (33, 3) and arrows.dtype == np.float64
    assert R.same(origins, p_m.astype(np.float64))
    assert R.same(arrows[0::2], origins) and R.same(arrows[1::2], origins)
    # and a non-zero one: the scale product first, then one multiply, then one add
    j = np.random.default_rng(3).uniform(-3, 3, (33, 3)).astype(F)
    arrows, _ = R.jacobian_points(p_m, j, 1.75)
    k = np.float64(1.75) * np.float64(0.05)
    for i in range(33):
        for a in range(3):
            assert arrows[2 * i + 1, a] == np.float64(j[i, a]) * k + np.float64(p_m[i, a])


def test_record_layout():
    p_m = np.array([[1.5, -2.25, 3.0], [0.1, 0.2, 0.3]], F)
    inten = np.array([0.75, -1e-3], F)
    rec = R.cloud_records(p_m, inten)
    assert rec.shape == (2, 32) and rec.dtype == np.uint8
    for i in range(2):
        b = rec[i].tobytes()
        assert np.frombuffer(b, F, 3, 0).tolist() == p_m[i].tolist()
        assert np.frombuffer(b, F, 1, 12)[0] == F(1.0)
        assert np.frombuffer(b, F, 1, 16)[0] == inten[i]
        assert b[20:] == bytes(12)


def test_point_transform_is_the_oracles():
    rng = np.random.default_rng(4)
    p = rng.uniform(-20, 20, (200, 3)).astype(F)
    for read_pose in ([1.5, -2.0, 0.3, 3.1], [-40.0, 7.0, -0.2, -3.12], [0.0, 0.0, 0.0, 0.0]):
        q, t = R.mission_pose(np.array(read_pose))
        assert q[1] == 0 and q[2] == 0 and t.tolist() == [float(F(v)) for v in read_pose[:3]]
        got = R.transform_points(q, t, p)
        want = np.stack([orc.transform_point(q, t, v) for v in p])
        assert R.same(got, want)


def test_exact_fixture_factors_are_powers_of_two():
    n = 1026
    assert R.factor_of(np.ones(n, F)) == 1.0
    assert R.factor_of(np.r_[np.full(n // 2, 0.25), np.full(n // 2, 0.75)].astype(F)) == 2.0
    assert R.factor_of(np.full(1025, 0.5, F)) == 2.0
    assert R.factor_of(None) == 1.0


def test_library_exports_the_visuals_entry_points():
    from voxgraph_amd import capi
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("vgx_reg_visuals_create", "vgx_reg_visuals_destroy", "vgx_reg_evaluate_visuals", "vgx_reg_visuals_stats",
                 "vgx_reg_visuals_download", "vgx_reg_visuals_device_pointers"):
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    assert "visualize_* are ignored" not in header
    assert "vgx_reg_evaluate_visuals" in header


def test_python_view_has_evaluate_visuals():
    from voxgraph_amd import capi
    assert callable(getattr(capi.RegistrationCostFunction, "evaluate_visuals"))
    assert capi.Registration is capi.RegistrationCostFunction
    for m in ("stats", "download", "device_pointers", "destroy"):
        assert callable(getattr(capi.RegVisuals, m))
