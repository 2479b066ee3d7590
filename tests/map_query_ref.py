"""CPU restatement of vgx_submap_query (include/voxgraph_amd.h): voxblox's EsdfMap / TsdfMap lookups -- nearest voxel,
trilinear interpolation, central-difference gradient -- at arbitrary points of one raw ESDF or TSDF layer, vectorised in
numpy f32.  Every numpy op rounds once, as the kernel's do under -ffp-contract=off, and the ops come in the kernel's
order, so results are comparable bit for bit.

A layer is anything with voxel_size, vps, block_index [n][3] and the raw arrays of oracle.synth.SubmapData
(tsdf_distance / tsdf_weight, esdf_distance / esdf_observed [n][vps^3])."""
import types

import numpy as np

from tests.projected_map_ref import EPS, F, RawLayer, inverse, quat_rotate

LIMIT = F(2.0 ** 30)  # |p * block_size_inv| at or above this (and every non-finite coordinate): an invalid query


class QueryLayer(RawLayer):
    """One raw layer of a submap: layer "esdf" (distance, observed != 0) or "tsdf" (distance, weight > 0).  RawLayer's
    neighbour rule and association serve both: for an ESDF its weight array holds observed as f32 (> 0 iff != 0), as
    the kernel's layer_interp reads the validity array."""

    def __init__(self, sm, layer="esdf"):
        self.tsdf = layer == "tsdf"
        if self.tsdf:
            d, w = sm.tsdf_distance, sm.tsdf_weight
        else:
            d, w = sm.esdf_distance, np.asarray(sm.esdf_observed, np.uint8).astype(F)
        super().__init__(types.SimpleNamespace(vps=sm.vps, voxel_size=sm.voxel_size, block_index=sm.block_index,
                                               tsdf_distance=d, tsdf_weight=w))

    def nearest(self, p):
        """getNearestDistance: p's own voxel -> (ok, distance, weight)"""
        vps = self.vps
        b, v = [], []
        for a in range(3):
            pa = p[..., a]
            b0 = np.floor((pa * self.bs_inv) + EPS).astype(np.int64)
            origin = (b0.astype(F) * self.bs).astype(F)
            b.append(b0)
            v.append(np.clip(np.floor(((pa - origin) * self.vs_inv) + EPS).astype(np.int64), 0, vps - 1))
        s = self.slot(np.stack(b, -1))
        lin = v[0] + vps * (v[1] + vps * v[2])
        sc = np.maximum(s, 0)
        d = np.where(s >= 0, self.d[sc, lin] if self.d.size else F(0), F(0)).astype(F)
        w = np.where(s >= 0, self.w[sc, lin] if self.w.size else F(0), F(0)).astype(F)
        return (s >= 0) & (w > F(0)), d, w

    def distance(self, p, interpolate):
        ok, d, w = self.interp(p) if interpolate else self.nearest(p)
        return ok, d, (w if self.tsdf else np.zeros_like(d))


def query(sm, points, layer="esdf", interpolate=True, gradient=False, pose=None):
    """vgx_submap_query -> (distance [n], gradient [n][3] or None, weight [n] (0 for an ESDF), valid [n] bool)."""
    L = QueryLayer(sm, layer)
    x = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if pose is not None:
            T = np.asarray(pose, F).reshape(7)
            qi, ti = inverse(T)
            p = (quat_rotate(qi, x) + ti).astype(F)
        else:
            p = x.copy()
        inside = (np.abs((p * L.bs_inv).astype(F)) < LIMIT).all(1)
        p = np.where(inside[:, None], p, F(0)).astype(F)  # (kept out of the integer casts; masked below)
        ok, d, w = L.distance(p, interpolate)
        g = None
        if gradient:
            dk = []
            for a in range(3):
                for s in (-1, 1):
                    q = p.copy()
                    q[:, a] = (p[:, a] - L.vs) if s < 0 else (p[:, a] + L.vs)
                    ok_k, d_k, _ = L.distance(q, interpolate)
                    ok &= ok_k
                    dk.append(d_k)
            two_vs = F(F(2) * L.vs)
            g = np.stack([((dk[2 * a + 1] - dk[2 * a]) / two_vs).astype(F) for a in range(3)], -1).astype(F)
            if pose is not None:
                g = quat_rotate(T[:4], g)
        ok &= inside
        d = np.where(ok, d, F(0)).astype(F)
        w = np.where(ok, w, F(0)).astype(F)
        if g is not None:
            g = np.where(ok[:, None], g, F(0)).astype(F)
    return d, g, w, ok
