"""CPU restatement of vgx_tsdf_layer_merge_submaps (include/voxgraph_amd.h): voxblox's mergeLayerAintoLayerB of each
submap's TSDF layer into one layer, vectorised in numpy f32.  Every numpy op below rounds once, as the kernel's do under
-ffp-contract=off, and the ops come in the kernel's order, so results are comparable bit for bit.

A layer here is a dict {(bx, by, bz): (distance[vps^3], weight[vps^3])} of f32 arrays; a submap is anything with
voxel_size, vps, block_index [n][3], tsdf_distance / tsdf_weight [n][vps^3] (oracle.synth.SubmapData)."""
import numpy as np

F = np.float32
EPS = F(1e-6)


def quat_rotate(q, v):
    """Eigen _transformVector: uv = 2 (u x v); v + w uv + u x uv.  q = (w, x, y, z) f32 scalars, v [..., 3] f32."""
    w, x, y, z = (F(c) for c in q)
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    u0 = y * v2 - z * v1
    u1 = z * v0 - x * v2
    u2 = x * v1 - y * v0
    u0 = u0 + u0
    u1 = u1 + u1
    u2 = u2 + u2
    c0 = y * u2 - z * u1
    c1 = z * u0 - x * u2
    c2 = x * u1 - y * u0
    return np.stack([(v0 + w * u0) + c0, (v1 + w * u1) + c1, (v2 + w * u2) + c2], -1).astype(F)


def transform(q, t, v):
    r = quat_rotate(q, v)
    return (r + np.asarray(t, F)).astype(F)


def inverse(T):
    """T.inverse() in f32: conjugate quaternion, translation -(q^-1 t)."""
    T = np.asarray(T, F)
    qi = np.array([T[0], -T[1], -T[2], -T[3]], F)
    ti = (-quat_rotate(qi, T[4:7].reshape(1, 3))[0]).astype(F)
    return qi, ti


def voxel_local(vps, voxel_size):
    """[vps^3, 3] (idx + 0.5) * voxel_size, voxblox linear order (x fastest)."""
    i = np.arange(vps ** 3)
    idx = np.stack([i % vps, (i // vps) % vps, i // (vps * vps)], -1).astype(F)
    return ((idx + F(0.5)) * F(voxel_size)).astype(F)


def block_centres(blocks, vps, voxel_size):
    """[m, vps^3, 3] voxel centres of layer blocks: origin + (idx + 0.5) * voxel_size."""
    bs = F(F(vps) * F(voxel_size))
    origin = (np.asarray(blocks, np.int64).astype(F) * bs).astype(F)
    return (origin[:, None, :] + voxel_local(vps, voxel_size)[None]).astype(F)


class RawLayer:
    """A submap's raw TSDF layer with a vectorised block lookup."""

    def __init__(self, sm):
        self.vps = int(sm.vps)
        self.vs = F(sm.voxel_size)
        self.vs_inv = F(F(1) / self.vs)
        self.bs = F(F(self.vps) * self.vs)
        self.bs_inv = F(F(1) / self.bs)
        self.bi = np.asarray(sm.block_index, np.int64).reshape(-1, 3)
        nv = self.vps ** 3
        self.d = np.asarray(sm.tsdf_distance, F).reshape(-1, nv)
        self.w = np.asarray(sm.tsdf_weight, F).reshape(-1, nv)
        keys = self._key(self.bi)
        self.order = np.argsort(keys)
        self.sorted = keys[self.order]

    @staticmethod
    def _key(b):
        b = np.asarray(b, np.int64) + (1 << 20)
        return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]

    def slot(self, b):
        """slot of block coordinates [..., 3], -1 if absent"""
        k = self._key(b)
        if self.sorted.size == 0:
            return np.full(k.shape, -1, np.int64)
        at = np.clip(np.searchsorted(self.sorted, k), 0, self.sorted.size - 1)
        return np.where(self.sorted[at] == k, self.order[at], -1)

    def interp(self, p):
        """Interpolator<TsdfVoxel>::getVoxel(p, &v, true) at points [..., 3] f32 -> (ok, distance, weight)."""
        vps = self.vps
        p = np.asarray(p, F)
        blk, vox, dl = [], [], []
        for a in range(3):
            pa = p[..., a]
            b0 = np.floor((pa * self.bs_inv) + EPS).astype(np.int64)
            origin = (b0.astype(F) * self.bs).astype(F)
            v = np.floor(((pa - origin) * self.vs_inv) + EPS).astype(np.int64)
            v = np.clip(v, 0, vps - 1)
            centre = (origin + ((v.astype(F) + F(0.5)) * self.vs)).astype(F)
            shift = (pa - centre) < F(0)
            v = np.where(shift, v - 1, v)
            wrap = v < 0
            b0 = np.where(wrap, b0 - 1, b0)
            v = np.where(wrap, v + vps, v)
            origin2 = (b0.astype(F) * self.bs).astype(F)
            dl.append(((pa - (origin2 + ((v.astype(F) + F(0.5)) * self.vs))) * self.vs_inv).astype(F))
            blk.append(b0)
            vox.append(v)
        ok = np.ones(p.shape[:-1], bool)
        d8, w8 = [], []
        for k in range(8):
            off = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
            nb, nv = [], []
            for a in range(3):
                v = vox[a] + off[a]
                nb.append(np.where(v >= vps, blk[a] + 1, blk[a]))
                nv.append(np.where(v >= vps, v - vps, v))
            s = self.slot(np.stack(nb, -1))
            lin = nv[0] + vps * (nv[1] + vps * nv[2])
            sc = np.maximum(s, 0)
            dk = np.where(s >= 0, self.d[sc, lin] if self.d.size else F(0), F(0)).astype(F)
            wk = np.where(s >= 0, self.w[sc, lin] if self.w.size else F(0), F(0)).astype(F)
            ok &= (s >= 0) & (wk > F(0))
            d8.append(dk)
            w8.append(wk)
        x, y, z = dl

        def tri(v):
            c0 = v[0]
            c1 = -v[0] + v[4]
            c2 = -v[0] + v[2]
            c3 = -v[0] + v[1]
            c4 = ((v[0] - v[2]) - v[4]) + v[6]
            c5 = ((v[0] - v[1]) - v[2]) + v[3]
            c6 = ((v[0] - v[1]) - v[4]) + v[5]
            c7 = ((((((-v[0] + v[1]) + v[2]) - v[3]) + v[4]) - v[5]) - v[6]) + v[7]
            q4, q5, q6, q7 = x * y, y * z, z * x, (x * y) * z
            return (((((((c0 + x * c1) + y * c2) + z * c3) + q4 * c4) + q5 * c5) + q6 * c6) + q7 * c7).astype(F)

        return ok, tri(d8), tri(w8)


def candidate_blocks(raw, T_L_S, vps, voxel_size):
    """A superset of the layer blocks a submap can reach: every block with data, grown by two voxels, into the layer."""
    has = (raw.w > F(0)).any(1)
    if not has.any():
        return np.zeros((0, 3), np.int64)
    bi = raw.bi[has]
    T = np.asarray(T_L_S, F)
    bs = float(F(F(vps) * F(voxel_size)))
    corners = np.array([[(k >> a) & 1 for a in range(3)] for k in range(8)], np.float64)
    lo_s = bi.astype(np.float64) * bs - 2 * float(voxel_size)
    pts = lo_s[:, None, :] + corners[None] * (bs + 4 * float(voxel_size))
    g = transform(T[:4], T[4:], pts.astype(F)).astype(np.float64)
    lo = np.floor(g.min(1) / bs).astype(np.int64)
    hi = np.floor(g.max(1) / bs).astype(np.int64)
    out = set()
    for l, h in zip(lo, hi):
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    out.add((x, y, z))
    return np.array(sorted(out), np.int64).reshape(-1, 3)


def merge_one(layer, sm, T_L_S, only=None):
    """mergeLayerAintoLayerB(sm's TSDF layer, T_L_S, layer), in place.  only: restrict to these target blocks."""
    vps, vs = int(sm.vps), F(sm.voxel_size)
    raw = RawLayer(sm)
    qi, ti = inverse(T_L_S)
    cand = candidate_blocks(raw, T_L_S, vps, vs)
    if only is not None:
        keep = {tuple(int(c) for c in b) for b in np.asarray(only).reshape(-1, 3)}
        cand = np.array([b for b in cand if tuple(int(c) for c in b) in keep], np.int64).reshape(-1, 3)
    for s in range(0, len(cand), 256):
        part = cand[s:s + 256]
        c = block_centres(part, vps, vs)
        p = transform(qi, ti, c)
        ok, d, w = raw.interp(p)
        contrib = ok.any(1)
        for b, o, db, wb in zip(part[contrib], ok[contrib], d[contrib], w[contrib]):
            key = tuple(int(v) for v in b)
            if key in layer:
                ld, lw = layer[key]
            else:
                ld = np.zeros(vps ** 3, F)
                lw = np.zeros(vps ** 3, F)
            da = np.where(o, db, F(0)).astype(F)
            wa = np.where(o, wb, F(0)).astype(F)
            layer[key] = merge_voxels(da, wa, ld, lw)
    return layer


def merge_voxels(da, wa, db, wb):
    """mergeVoxelAIntoVoxelB: w' = wA + wB; if w' > 0: d = (dA wA + dB wB) / w', w = w'."""
    wn = (wa + wb).astype(F)
    pos = wn > F(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = (((da * wa) + (db * wb)) / wn).astype(F)
    return np.where(pos, dn, db).astype(F), np.where(pos, wn, wb).astype(F)


def merge_submaps(layer, submaps, T_L_S, only=None):
    """vgx_tsdf_layer_merge_submaps restated: submaps in array order."""
    T = np.asarray(T_L_S, F).reshape(-1, 7)
    for sm, t in zip(submaps, T):
        merge_one(layer, sm, t, only)
    return layer


def layer_from_arrays(block_index, distance, weight):
    return {tuple(int(v) for v in b): (np.asarray(d, F).copy(), np.asarray(w, F).copy())
            for b, d, w in zip(np.asarray(block_index).reshape(-1, 3), distance, weight)}
