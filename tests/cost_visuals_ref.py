"""numpy restatement of the cost-function visuals (include/voxgraph_amd.h, "Cost-function visuals"): what
RegistrationCostFunction::Evaluate hands to CostFunctionVisuals (registration_cost_function.cpp:169-176, 244-252, 293-295;
cost_function_visuals.cpp:43-101), from the SCALED f64 rows an evaluation returns.

TEST INFRASTRUCTURE.  The rows are scaled by factor = num_residuals / summed_weight in f64; the visuals are built from
the unscaled f32 values.  With a power-of-two factor rows / factor is exact, so the restatement recovers r_u and j bit
for bit (`factor_of` says what the factor is; the exact fixtures check that it is 1.0 or 2.0)."""
import numpy as np

from oracle import pyoracle as orc

F = np.float32
POINT_STEP = 32
FRAME = "mission"
CHILD_FRAME = "optimized_submap"
LINE_LIST, SPHERE_LIST = 5, 7
ARROWS = dict(ns="jacobian_vectors", id=1, type=LINE_LIST, scale=(0.02, 0.0, 0.0), color=(1.0, 0.0, 0.0, 1.0))
ORIGINS = dict(ns="jacobian_origins", id=2, type=SPHERE_LIST, scale=(0.05, 0.05, 0.05), color=(0.0, 0.0, 0.0, 1.0))


def factor_of(weights=None, n=None):
    """num_residuals / summed_weight with the weights summed sequentially in f64 (RCF:124, 274); sampling: 1.0"""
    if weights is None:
        return 1.0
    acc = 0.0
    for v in np.asarray(weights, F).astype(np.float64):
        acc += v
    n = len(weights) if n is None else n
    return float(np.float64(n) / np.float64(acc))


def mission_pose(read_pose):
    """T_mission__reading (RCF:80-88) as (q wxyz f32, t f32): the oracle's relative transform of the pose against the
    identity (1 * q and 0 + t are exact)"""
    return orc.relative_transform(read_pose, np.zeros(4))


def transform_points(q, t, p):
    """minkindr's point transform q * p + t over rows, in f32, one rounding per operation (Eigen _transformVector:
    uv = 2 u x v; v + w uv + u x uv): the algebra of oracle.pyoracle.transform_point"""
    q = np.asarray(q, F)
    t = np.asarray(t, F)
    p = np.asarray(p, F).reshape(-1, 3)
    w, x, y, z = q[0], q[1], q[2], q[3]
    v0, v1, v2 = p[:, 0], p[:, 1], p[:, 2]
    uv0 = y * v2 - z * v1
    uv1 = z * v0 - x * v2
    uv2 = x * v1 - y * v0
    uv0 = uv0 + uv0
    uv1 = uv1 + uv1
    uv2 = uv2 + uv2
    c0 = y * uv2 - z * uv1
    c1 = z * uv0 - x * uv2
    c2 = x * uv1 - y * uv0
    r0 = v0 + w * uv0 + c0
    r1 = v1 + w * uv1 + c1
    r2 = v2 + w * uv2 + c2
    out = np.stack([r0 + t[0], r1 + t[1], r2 + t[2]], -1)
    assert out.dtype == F
    return out


def mission_points(xyz, ref_pose, read_pose):
    """p_m = T_mission__reading * (T_reading__reference * p_ref), f32"""
    q_rel, t_rel = orc.relative_transform(ref_pose, read_pose)
    q_m, t_m = mission_pose(read_pose)
    return transform_points(q_m, t_m, transform_points(q_rel, t_rel, xyz))


def intensity(r_unscaled, factor):
    """CFV:49 narrows the unscaled residual to float, CFV:75 multiplies it by the double factor in f64, rounded once"""
    return (np.asarray(r_unscaled, np.float64).astype(F).astype(np.float64) * np.float64(factor)).astype(F)


def cloud_records(p_m, inten):
    """[n][32] u8: pcl::PointXYZI -- x y z at bytes 0 4 8, 1.0f at 12, intensity at 16, the rest zero"""
    n = len(p_m)
    rec = np.zeros((n, 8), F)
    rec[:, 0:3] = p_m
    rec[:, 3] = F(1.0)
    rec[:, 4] = inten
    return rec.view(np.uint8).reshape(n, POINT_STEP)


def jacobian_points(p_m, j, factor):
    """(arrow points [2n][3] f64 = o0 t0 o1 t1 .., origin points [n][3] f64): t = f64(j) * (factor * 0.05) + o, the
    scale product first, then one multiply and one add per component (CFV:82-89)"""
    o = np.asarray(p_m, F).astype(np.float64)
    scale = np.float64(factor) * np.float64(0.05)
    scaled = np.asarray(j, F).astype(np.float64) * scale
    tip = scaled + o
    arrows = np.empty((2 * len(o), 3), np.float64)
    arrows[0::2] = o
    arrows[1::2] = tip
    return arrows, o


def visuals(xyz, rows_r, rows_jac_read, factor, ref_pose, read_pose):
    """The three arrays of one evaluation from its scaled rows: xyz [n][3] the points of the rows in row order (the drawn
    points when sampling), rows_r [n] f64, rows_jac_read [n][4] f64 or None (no Jacobians asked for: no markers).
    Returns (cloud [n][32] u8, arrows [2m][3] f64, origins [m][3] f64)."""
    p_m = mission_points(xyz, ref_pose, read_pose)
    r_u = np.asarray(rows_r, np.float64) / np.float64(factor)
    cloud = cloud_records(p_m, intensity(r_u, factor))
    if rows_jac_read is None:
        return cloud, np.zeros((0, 3)), np.zeros((0, 3))
    j = (np.asarray(rows_jac_read, np.float64)[:, :3] / np.float64(factor)).astype(F)
    arrows, origins = jacobian_points(p_m, j, factor)
    return cloud, arrows, origins


def same(a, b):
    """bit for bit, on an unsigned view"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(view), b.view(view)))


def ulp_distance_f32(a, b):
    """|a - b| in units of f32 steps (monotone integer mapping of the bit patterns)"""
    def key(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
