"""Voxel colours through the map products, restated in numpy: the colour rules of vgx_tsdf_layer_merge_submaps /
vgx_tsdf_layer_transform_submap, vgx_*_generate_mesh_colored (MeshIntegrator::updateMeshColor) and the per-vertex layout
of vgx_mesh_fill_marker / vgx_mesh_connect (include/voxgraph_amd.h).  Every numpy op rounds once, in the kernels' order,
so the device is compared with this bit for bit (tests/test_map_colour_gpu.py); tests/test_map_colour_cpu.py checks the
restatement itself.  Where a rule is already stated elsewhere it is taken from there: projected_map_ref (poses, block
candidates, the distance merge), map_msg_ref (blendTwoColors), connected_mesh_ref (the weld), mesh_marker_ref (shading).

A coloured layer here is a dict {(bx, by, bz): (distance [nv] f32, weight [nv] f32, rgba [nv][4] u8)}; a submap is
anything with voxel_size, vps, block_index, tsdf_distance, tsdf_weight and tsdf_rgba ([n][nv][4] u8, or None: a submap
without colours)."""
import numpy as np

from tests import connected_mesh_ref as cmr
from tests import map_msg_ref as mm
from tests import mesh_marker_ref as mk
from tests import projected_map_ref as pm

F = np.float32
EPS = pm.EPS


def trilinear(v, x, y, z):
    """interp_trilinear (vgx_interp.h) over 8 neighbour arrays v[k] (k: x = bit 2, y = bit 1, z = bit 0)"""
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


def clamp_trunc(v):
    """the stated float -> byte conversion of an interpolated channel: clamped to [0, 255], then truncated toward zero"""
    return np.trunc(np.clip(np.asarray(v, F), F(0), F(255))).astype(np.uint8)


def interp_channels(c8, x, y, z):
    """c8: 8 arrays [..., 4] u8 in neighbour order -> (bytes [..., 4] u8, the f32 values before the clamp [..., 4])"""
    raw = np.stack([trilinear([c[..., ch].astype(F) for c in c8], x, y, z) for ch in range(4)], -1)
    return clamp_trunc(raw), raw


def blended_color(c_old, c_new, w_old, w_new):
    """blended_color (vgx_tsdf_internal.h), Color::blendTwoColors: map_msg_ref states it"""
    return mm.blend(c_old, c_new, w_old, w_new)


class ColourLayer(pm.RawLayer):
    """pm.RawLayer plus the voxels' colours"""

    def __init__(self, sm):
        super().__init__(sm)
        rgba = getattr(sm, "tsdf_rgba", None)
        self.rgba = None if rgba is None else np.ascontiguousarray(rgba, np.uint8).reshape(-1, self.vps ** 3, 4)

    def base(self, p):
        """interp_base per axis: (blk, vox, dl) lists of three arrays"""
        vps = self.vps
        blk, vox, dl = [], [], []
        for a in range(3):
            pa = p[..., a]
            b0 = np.floor((pa * self.bs_inv) + EPS).astype(np.int64)
            origin = (b0.astype(F) * self.bs).astype(F)
            v = np.clip(np.floor(((pa - origin) * self.vs_inv) + EPS).astype(np.int64), 0, vps - 1)
            centre = (origin + ((v.astype(F) + F(0.5)) * self.vs)).astype(F)
            v = np.where((pa - centre) < F(0), v - 1, v)
            wrap = v < 0
            b0 = np.where(wrap, b0 - 1, b0)
            v = np.where(wrap, v + vps, v)
            origin2 = (b0.astype(F) * self.bs).astype(F)
            dl.append(((pa - (origin2 + ((v.astype(F) + F(0.5)) * self.vs))) * self.vs_inv).astype(F))
            blk.append(b0)
            vox.append(v)
        return blk, vox, dl

    def interp_coloured(self, p):
        """Interpolator<TsdfVoxel>::getVoxel(p, &v, true) with the colour: (ok, distance, weight, rgba [..., 4] u8, the
        channels before the clamp [..., 4] f32).  rgba is zeros where ok is false or the layer has no colours."""
        vps = self.vps
        p = np.asarray(p, F)
        blk, vox, dl = self.base(p)
        ok = np.ones(p.shape[:-1], bool)
        d8, w8, c8 = [], [], []
        for k in range(8):
            off = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
            nb = [np.where(vox[a] + off[a] >= vps, blk[a] + 1, blk[a]) for a in range(3)]
            nv = [np.where(vox[a] + off[a] >= vps, vox[a] + off[a] - vps, vox[a] + off[a]) for a in range(3)]
            s = self.slot(np.stack(nb, -1))
            lin = nv[0] + vps * (nv[1] + vps * nv[2])
            sc = np.maximum(s, 0)
            have = s >= 0
            dk = np.where(have, self.d[sc, lin] if self.d.size else F(0), F(0)).astype(F)
            wk = np.where(have, self.w[sc, lin] if self.w.size else F(0), F(0)).astype(F)
            ok &= have & (wk > F(0))
            d8.append(dk)
            w8.append(wk)
            if self.rgba is not None and self.rgba.size:
                c8.append(np.where(have[..., None], self.rgba[sc, lin], np.uint8(0)).astype(np.uint8))
        x, y, z = dl
        d, w = trilinear(d8, x, y, z), trilinear(w8, x, y, z)
        if c8:
            c, raw = interp_channels(c8, x, y, z)
            c = np.where(ok[..., None], c, np.uint8(0)).astype(np.uint8)
        else:
            c, raw = np.zeros(p.shape[:-1] + (4,), np.uint8), np.zeros(p.shape[:-1] + (4,), F)
        return ok, d, w, c, raw


def _candidates(raw, T, only):
    cand = pm.candidate_blocks(raw, T, raw.vps, raw.vs)
    if only is not None:
        keep = {tuple(int(c) for c in b) for b in np.asarray(only).reshape(-1, 3)}
        cand = np.array([b for b in cand if tuple(int(c) for c in b) in keep], np.int64).reshape(-1, 3)
    return cand


def merge_one(layer, sm, T_L_S, only=None, copy=False):
    """mergeLayerAintoLayerB with colour (copy: transformLayer's COPY into the empty layer), in place"""
    raw = ColourLayer(sm)
    vps, nv = raw.vps, raw.vps ** 3
    qi, ti = pm.inverse(T_L_S)
    cand = _candidates(raw, T_L_S, only)
    coloured = raw.rgba is not None
    for s in range(0, len(cand), 256):
        part = cand[s:s + 256]
        p = pm.transform(qi, ti, pm.block_centres(part, vps, raw.vs))
        ok, d, w, c, _ = raw.interp_coloured(p)
        contrib = ok.any(1)
        for b, o, db, wb, cb in zip(part[contrib], ok[contrib], d[contrib], w[contrib], c[contrib]):
            key = tuple(int(v) for v in b)
            ld, lw, lc = layer.get(key, (np.zeros(nv, F), np.zeros(nv, F), np.zeros((nv, 4), np.uint8)))
            da = np.where(o, db, F(0)).astype(F)
            wa = np.where(o, wb, F(0)).astype(F)
            ca = np.where(o[:, None], cb, np.uint8(0)).astype(np.uint8)     # the default voxel: colour 0, w = 0
            if copy:
                layer[key] = (da, wa, ca if coloured else lc)
                continue
            nd, nw = pm.merge_voxels(da, wa, ld, lw)
            if coloured:
                upd = (wa + lw).astype(F) > F(0)                            # where the rule updates the voxel
                lc = np.where(upd[:, None], blended_color(lc, ca, lw, wa), lc).astype(np.uint8)
            layer[key] = (nd, nw, lc)
    return layer


def merge_submaps(layer, submaps, T_L_S, only=None):
    """vgx_tsdf_layer_merge_submaps with colours restated: submaps in array order, with and without colours mixed"""
    for sm, t in zip(submaps, np.asarray(T_L_S, F).reshape(-1, 7)):
        merge_one(layer, sm, t, only)
    return layer


def transform_submap(sm, T_L_S):
    """vgx_tsdf_layer_transform_submap into an empty layer"""
    return merge_one({}, sm, np.asarray(T_L_S, F).reshape(7), copy=True)


def layer_from_arrays(block_index, distance, weight, rgba):
    nv = np.asarray(distance).shape[-1] if len(np.asarray(block_index).reshape(-1, 3)) else 0
    return {tuple(int(v) for v in b): (np.asarray(d, F).copy(), np.asarray(w, F).copy(),
                                       np.asarray(c, np.uint8).reshape(nv, 4).copy())
            for b, d, w, c in zip(np.asarray(block_index).reshape(-1, 3), distance, weight, rgba)}


def nearest_voxel(p, block, vps, voxel_size):
    """updateMeshColor's voxel of vertices p [N][3] f32 that belong to triangles of blocks block [N][3]:
    (block [N][3] int64, voxel [N][3] int64, moved [N] bool: taken from another block than the triangle's)"""
    vs = F(voxel_size)
    vsi = F(F(1) / vs)
    bs = F(F(vps) * vs)
    bsi = F(F(1) / bs)
    p = np.asarray(p, F).reshape(-1, 3)
    block = np.asarray(block, np.int64).reshape(-1, 3)
    origin = (block.astype(F) * bs).astype(F)
    with np.errstate(invalid="ignore"):
        v = np.floor(((p - origin) * vsi) + EPS).astype(np.int64)
        inside = ((v >= 0) & (v < vps)).all(1)
        nb = np.floor((p * bsi) + EPS).astype(np.int64)
        origin2 = (nb.astype(F) * bs).astype(F)
        v2 = np.clip(np.floor(((p - origin2) * vsi) + EPS).astype(np.int64), 0, vps - 1)
    out_b = np.where(inside[:, None], block, nb)
    out_v = np.where(inside[:, None], v, v2)
    return out_b, out_v, (out_b != block).any(1)


def vertex_colours(mesh_blocks, first, vertices, block_index, weight, rgba, vps, voxel_size, min_weight=1e-4):
    """MeshIntegrator::updateMeshColor restated: mesh_blocks [nb][3] / first [nb+1] / vertices [T][3][3] as the mesh holds
    them; block_index [n][3], weight [n][nv], rgba [n][nv][4] the TSDF source.  Returns (rgba [T][3][4] u8, moved [T][3])."""
    v = np.asarray(vertices, F).reshape(-1, 3, 3)
    T = len(v)
    if T == 0:
        return np.zeros((0, 3, 4), np.uint8), np.zeros((0, 3), bool)
    k = np.searchsorted(np.asarray(first, np.int64), np.arange(T), side="right") - 1
    blk = np.repeat(np.asarray(mesh_blocks, np.int64).reshape(-1, 3)[k], 3, axis=0)
    b, vox, moved = nearest_voxel(v.reshape(-1, 3), blk, vps, voxel_size)
    row = {tuple(int(c) for c in x): i for i, x in enumerate(np.asarray(block_index, np.int64).reshape(-1, 3))}
    slot = np.array([row.get(tuple(int(c) for c in x), -1) for x in b], np.int64)
    lin = vox[:, 0] + vps * (vox[:, 1] + vps * vox[:, 2])
    sc = np.maximum(slot, 0)
    w = np.asarray(weight, F).reshape(-1, vps ** 3)[sc, lin]
    valid = (slot >= 0) & (w >= F(min_weight))                               # getColorIfValid
    c = np.asarray(rgba, np.uint8).reshape(-1, vps ** 3, 4)[sc, lin]
    return np.where(valid[:, None], c, np.uint8(0)).astype(np.uint8).reshape(T, 3, 4), moved.reshape(T, 3)


def fill_marker(vertices, normals, vertex_rgba, mode, opacity=1.0):
    """vgx_mesh_fill_marker on a per-vertex mesh, COLOR or LAMBERT_COLOR: each vertex through mesh_marker_ref's c8 table
    and formulas with its own colour and its triangle's normal.  Returns (points [3T][3] f64, colors [3T][4] f32)."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3, 3)
    n3 = np.repeat(np.ascontiguousarray(normals, F).reshape(-1, 3), 3, axis=0)
    # one "triangle" per vertex: its own colour, its triangle's normal
    rgb = mk.triangle_rgb(n3, np.asarray(vertex_rgba, np.uint8).reshape(-1, 4), mode)
    colors = np.empty((3 * len(v), 4), F)
    colors[:, :3] = rgb
    colors[:, 3] = F(opacity)
    return v.reshape(-1, 3).astype(np.float64), colors


def connect(vertices, normals, vertex_rgba, threshold=cmr.DEFAULT_THRESHOLD):
    """vgx_mesh_connect on a per-vertex mesh: connected_mesh_ref's weld, a welded vertex taking the colour of its first
    soup vertex.  Returns (vertices [V][3], normals [V][3], rgba [V][4], indices [T][3])."""
    cv, cn, _, idx = cmr.connect(vertices, normals, None, threshold)
    flat = idx.ravel().astype(np.int64)
    if len(flat) == 0:
        return cv, cn, np.zeros((0, 4), np.uint8), idx
    _, rep = np.unique(flat, return_index=True)                              # first soup vertex of each unique vertex
    return cv, cn, np.asarray(vertex_rgba, np.uint8).reshape(-1, 4)[rep], idx


def read_ply(path):
    """a binary_little_endian PLY as vgx_mesh_write_ply / vgx_connected_mesh_write_ply write it ->
    (vertex records as a structured array, faces [T][3] int32)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().split("\n")
    nv = next(int(h.split()[2]) for h in header if h.startswith("element vertex"))
    nf = next(int(h.split()[2]) for h in header if h.startswith("element face"))
    fields = [(h.split()[2], {"float": "<f4", "uchar": "u1"}[h.split()[1]]) for h in header
              if h.startswith("property") and "list" not in h]
    vt = np.dtype(fields)
    verts = np.frombuffer(data, vt, nv, end)
    ft = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    faces = np.frombuffer(data, ft, nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(data) and (faces["n"] == 3).all()
    return verts, faces["i"]
