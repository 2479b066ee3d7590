"""Numpy restatement of the map messages (include/voxgraph_amd.h, "Map messages"): the block words of
voxblox::serializeLayerAsMsg, the three actions of deserializeMsgToLayer with mergeVoxelAIntoVoxelB and the colour blend,
and the data bytes of publishSubmapSurfacePointcloud's pcl::PointXYZI cloud with pcl::transformPoint.  Everything in f32,
one operation at a time (numpy never contracts)."""
import numpy as np

F = np.float32
U = np.uint32
TSDF_WORDS, ESDF_WORDS = 3, 2
UPDATE, MERGE, RESET = 0, 1, 2          # voxblox MapDerializationAction [recalled]
POINT_STEP = 32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def colour_word(rgba):
    """bytes r g b a [..., 4] -> a | b << 8 | g << 16 | r << 24"""
    c = np.asarray(rgba, np.uint8).astype(U)
    return c[..., 3] | (c[..., 2] << U(8)) | (c[..., 1] << U(16)) | (c[..., 0] << U(24))


def colour_bytes(word):
    w = np.asarray(word, U)
    return np.stack([w >> U(24), (w >> U(16)) & U(255), (w >> U(8)) & U(255), w & U(255)], -1).astype(np.uint8)


def tsdf_words(distance, weight, rgba=None):
    """[n][nv] f32, f32, [n][nv][4] u8 or None (colour word 0) -> [n][nv * 3] u32"""
    d = np.ascontiguousarray(distance, F)
    n, nv = d.shape
    out = np.zeros((n, nv, 3), U)
    out[:, :, 0] = d.view(U)
    out[:, :, 1] = np.ascontiguousarray(weight, F).view(U)
    if rgba is not None:
        out[:, :, 2] = colour_word(np.asarray(rgba, np.uint8).reshape(n, nv, 4))
    return out.reshape(n, nv * 3)


def esdf_words(distance, observed):
    d = np.ascontiguousarray(distance, F)
    n, nv = d.shape
    out = np.zeros((n, nv, 2), U)
    out[:, :, 0] = d.view(U)
    out[:, :, 1] = (np.asarray(observed).reshape(n, nv) != 0).astype(U)
    return out.reshape(n, nv * 2)


def tsdf_decode(words):
    """[n][nv * 3] u32 -> distance, weight [n][nv] f32, rgba [n][nv][4] u8"""
    w = np.ascontiguousarray(words, U)
    w = w.reshape(w.shape[0], -1, 3)
    return (np.ascontiguousarray(w[:, :, 0]).view(F), np.ascontiguousarray(w[:, :, 1]).view(F), colour_bytes(w[:, :, 2]))


def esdf_decode(words):
    w = np.ascontiguousarray(words, U)
    w = w.reshape(w.shape[0], -1, 2)
    return np.ascontiguousarray(w[:, :, 0]).view(F), ((w[:, :, 1] & U(255)) != 0).astype(np.uint8)


def _roundf(x):
    """roundf for x >= 0: half away from zero (np.round goes to even)"""
    t = np.trunc(x)
    return t + ((x - t) >= F(0.5)).astype(F)


def blend(c_old, c_new, w_old, w_new):
    """Color::blendTwoColors as the integrators form it (vgx_tsdf_internal.h blended_color): bytes [..., 4], f32 weights"""
    w_old, w_new = np.asarray(w_old, F), np.asarray(w_new, F)
    with np.errstate(all="ignore"):
        total = w_old + w_new
        fw, sw = (w_old / total)[..., None], (w_new / total)[..., None]
        v = _roundf(np.asarray(c_old, np.uint8).astype(F) * fw + np.asarray(c_new, np.uint8).astype(F) * sw)
        return np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0).clip(0, 255).astype(np.uint8)


def merge_voxels(dA, wA, cA, dB, wB, cB):
    """mergeVoxelAIntoVoxelB(A = message voxel, B = layer voxel) -> the new B"""
    dA, wA, dB, wB = (np.asarray(x, F) for x in (dA, wA, dB, wB))
    with np.errstate(all="ignore"):
        wn = wA + wB
        hit = wn > F(0)                                   # (a NaN sum is not > 0: unchanged)
        d = np.where(hit, (dA * wA + dB * wB) / wn, dB).astype(F)
        # where the guard fails the old bits stay, NaN payloads included
        d = np.where(hit, d.view(U), dB.view(U)).astype(U).view(F)
        w = np.where(hit, wn.view(U), wB.view(U)).astype(U).view(F)
        c = np.where(hit[..., None], blend(cB, cA, wB, wA), np.asarray(cB, np.uint8))
    return d, w, c.astype(np.uint8)


def as_dict(bi, d, w, rgba):
    """a layer as {block index: (distance [nv], weight [nv], rgba [nv][4])}"""
    rgba = np.asarray(rgba, np.uint8).reshape(len(bi), np.asarray(d).shape[1] if len(bi) else 0, 4)
    return {tuple(int(v) for v in bi[k]): (np.array(d[k], F), np.array(w[k], F), np.array(rgba[k], np.uint8)) for k in range(len(bi))}


def deserialize(layer, action, bi, words):
    """deserializeMsgToLayer on a layer dict (as_dict); returns the new dict"""
    out = {} if action == RESET else {k: tuple(a.copy() for a in v) for k, v in layer.items()}
    d, w, c = tsdf_decode(words) if len(bi) else (np.zeros((0, 0), F),) * 2 + (np.zeros((0, 0, 4), np.uint8),)
    for k in range(len(bi)):
        key = tuple(int(v) for v in bi[k])
        if action == MERGE and key in out:
            out[key] = merge_voxels(d[k], w[k], c[k], *out[key])
        else:
            out[key] = (d[k].copy(), w[k].copy(), c[k].copy())
    return out


def same_layers(a, b):
    return set(a) == set(b) and all(same(a[k][i], b[k][i]) for k in a for i in range(3))


def transform_points(xyz, T):
    """pcl::transformPoint with a row-major 3 x 4 affine: per row ((m0 x + m1 y) + m2 z) + t"""
    p, m = np.ascontiguousarray(xyz, F), np.asarray(T, F).reshape(3, 4)
    return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], -1).astype(F)


def surface_bytes(xyz, weight, T=None):
    """[n][3] f32, [n] f32 -> [n][32] u8: x y z 1.0f | intensity = weight, 12 zero bytes"""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    if T is not None:
        p = transform_points(p, T)
    out = np.zeros((len(p), 8), U)
    out[:, 0:3] = p.view(U)
    out[:, 3] = F(1.0).view(U)
    out[:, 4] = np.ascontiguousarray(weight, F).view(U)
    return out.view(np.uint8).reshape(len(p), POINT_STEP)
