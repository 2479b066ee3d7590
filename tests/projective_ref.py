"""numpy restatement of projective depth-image integration (include/voxgraph_amd.h, "Projective depth-image
integration"): the candidate block box (f64), every per-voxel rule in np.float32 -- one rounding per operation, the
header's operation order -- the running average, the colour blend and the slot order of new blocks.  Needs no device."""
import numpy as np

F = np.float32
DEPTH_16UC1, DEPTH_32FC1 = 0, 1
COLOR_NONE, COLOR_RGB8, COLOR_BGR8, COLOR_RGBA8, COLOR_BGRA8, COLOR_MONO8 = range(6)
DEPTH_BPP = {DEPTH_16UC1: 2, DEPTH_32FC1: 4}
COLOR_BPP = {COLOR_NONE: 0, COLOR_RGB8: 3, COLOR_BGR8: 3, COLOR_RGBA8: 4, COLOR_BGRA8: 4, COLOR_MONO8: 1}
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -4      # (the header's VGX_OK, VGX_ERR_INVALID, VGX_ERR_UNSUPPORTED)

# what a voxel of a candidate block met (Frame.branch): the first rule that decided
NO_PIXEL, INVALID_DEPTH, TOO_SHORT, CLEAR_REFUSED, BEHIND, CARVE_REFUSED, NO_CHANGE, UPDATED, CARVED, CLEARED = range(10)


class Config:
    """the vgx_tsdf_config fields the projective integrator reads (voxblox's defaults)"""

    def __init__(self, **kw):
        self.default_truncation_distance, self.max_weight, self.voxel_carving_enabled = 0.1, 10000.0, 1
        self.min_ray_length_m, self.max_ray_length_m, self.use_const_weight = 0.1, 5.0, 0
        self.allow_clear, self.use_weight_dropoff = 1, 1
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def capi(self, capi, **more):
        return capi.tsdf_config(**{**self.__dict__, **more})


class Camera:
    def __init__(self, fx, fy, cx, cy, depth_unit_m=0.001, min_depth_m=0.0, max_depth_m=np.inf):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.depth_unit_m, self.min_depth_m, self.max_depth_m = depth_unit_m, min_depth_m, max_depth_m

    def capi(self, capi, **more):
        return capi.depth_camera(**{**self.__dict__, **more})


class Image:
    """a depth frame's bytes and its registered colour image's, as a driver publishes them"""

    def __init__(self, width, height, encoding, depth, row_step=None, color_kind=COLOR_NONE, color=None, color_row_step=None):
        self.width, self.height, self.encoding, self.color_kind = width, height, encoding, color_kind
        self.row_step = width * DEPTH_BPP[encoding] if row_step is None else row_step
        self.color_row_step = width * COLOR_BPP[color_kind] if color_row_step is None else color_row_step
        self.depth = np.ascontiguousarray(depth, np.uint8).reshape(-1)
        self.color = None if color is None else np.ascontiguousarray(color, np.uint8).reshape(-1)

    def layout(self, capi):
        return capi.depth_image_layout(width=self.width, height=self.height, row_step=self.row_step, encoding=self.encoding,
                                       color_kind=self.color_kind, color_row_step=self.color_row_step)

    def z(self, cam):
        """[height][width] f32: the decode's depth rule"""
        bpp = DEPTH_BPP[self.encoding]
        at = (np.arange(self.height)[:, None] * self.row_step + np.arange(self.width)[None, :] * bpp)[..., None] + np.arange(bpp)
        b = self.depth[at]
        if self.encoding == DEPTH_16UC1:
            raw = b[..., 0].astype(np.uint32) | (b[..., 1].astype(np.uint32) << 8)
            return raw.astype(F) * F(cam.depth_unit_m)
        return np.ascontiguousarray(b).view("<f4")[..., 0]

    def rgba(self):
        """[height][width] u32 (bytes r g b a, r lowest): the decode's colour rule; NONE: opaque white"""
        if self.color_kind == COLOR_NONE:
            return np.full((self.height, self.width), 0xffffffff, np.uint32)
        bpp = COLOR_BPP[self.color_kind]
        at = (np.arange(self.height)[:, None] * self.color_row_step + np.arange(self.width)[None, :] * bpp)[..., None] + np.arange(bpp)
        b = self.color[at].astype(np.uint32)
        if bpp == 1:
            r = g = bl = b[..., 0]
            a = np.full_like(r, 255)
        else:
            bgr = self.color_kind in (COLOR_BGR8, COLOR_BGRA8)
            r, g, bl = (b[..., 2] if bgr else b[..., 0]), b[..., 1], (b[..., 0] if bgr else b[..., 2])
            a = b[..., 3] if bpp == 4 else np.full_like(r, 255)
        return r | (g << 8) | (bl << 16) | (a << 24)


def box(width, height, cam, cfg, T, voxel_size, vps):
    """vgx_tsdf_projective_box: (code, lo, hi); f64 throughout, the header's operation order"""
    T = np.asarray(T, F).astype(np.float64)
    if not np.isfinite(T).all():
        return ERR_INVALID, None, None
    if width >= 1 << 24 or height >= 1 << 24:
        return ERR_UNSUPPORTED, None, None
    trunc = float(F(cfg.default_truncation_distance))
    reach = min(float(F(cam.max_depth_m)), float(F(cfg.max_ray_length_m))) + trunc
    if not np.isfinite(reach) or not reach > 0.0:
        return ERR_UNSUPPORTED, None, None
    bs = float(F(voxel_size)) * float(vps)
    qw, qx, qy, qz = T[:4]
    mn, mx = T[4:].copy(), T[4:].copy()
    for corner in range(4):
        u = width - 0.5 if corner & 1 else -0.5
        v = height - 0.5 if corner & 2 else -0.5
        px, py, pz = ((u - cam.cx) / cam.fx) * reach, ((v - cam.cy) / cam.fy) * reach, reach
        uvx, uvy, uvz = qy * pz - qz * py, qz * px - qx * pz, qx * py - qy * px
        uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
        ccx, ccy, ccz = qy * uvz - qz * uvy, qz * uvx - qx * uvz, qx * uvy - qy * uvx
        g = np.array([(px + qw * uvx + ccx) + T[4], (py + qw * uvy + ccy) + T[5], (pz + qw * uvz + ccz) + T[6]])
        mn, mx = np.minimum(mn, g), np.maximum(mx, g)
    flo, fhi = np.floor(mn / bs) - 1.0, np.floor(mx / bs) + 1.0
    if not ((flo > -2.0 ** 30).all() and (fhi < 2.0 ** 30).all()):
        return ERR_UNSUPPORTED, None, None
    return OK, flo.astype(np.int32), fhi.astype(np.int32)


def _roundf(x):
    """roundf of non-negative f32 values (half away from zero), exactly"""
    return np.floor(x.astype(np.float64) + 0.5)


def blend(oc, color, old_w, w):
    """Color::blendTwoColors on packed words (vgx_tsdf_internal.h blended_color)"""
    total = old_w + w
    fw, sw = old_w / total, w / total
    out = np.zeros_like(oc)
    for k in range(4):
        a, b = ((oc >> (8 * k)) & 0xff).astype(F), ((color >> (8 * k)) & 0xff).astype(F)
        out |= (_roundf(a * fw + b * sw).astype(np.uint32) & 0xff) << np.uint32(8 * k)
    return out


class Layer:
    """a TSDF layer as vgx_tsdf_layer_download returns it: blocks in slot order"""

    def __init__(self, voxel_size, vps):
        self.voxel_size, self.vps = voxel_size, vps
        self.index = {}
        self.block_index = np.zeros((0, 3), np.int32)
        self.distance = np.zeros((0, vps ** 3), F)
        self.weight = np.zeros((0, vps ** 3), F)
        self.rgba = np.zeros((0, vps ** 3), np.uint32)

    @classmethod
    def of(cls, voxel_size, vps, block_index, distance, weight, rgba):
        L = cls(voxel_size, vps)
        L.block_index = np.array(block_index, np.int32).reshape(-1, 3)
        L.distance, L.weight = np.array(distance, F), np.array(weight, F)
        L.rgba = np.ascontiguousarray(rgba, np.uint8).reshape(len(L.block_index), vps ** 3, 4).view(np.uint32)[..., 0].copy()
        L.index = {tuple(b): i for i, b in enumerate(L.block_index.tolist())}
        return L

    def download(self):
        return self.block_index, self.distance, self.weight, self.rgba[..., None].view(np.uint8).reshape(len(self.rgba), self.vps ** 3, 4)   # (no -1: a layer without blocks)


class Frame:
    """what integrate() found: the counts, and per voxel of every candidate block the branch it took"""


def integrate(L, T, img, cam, cfg):
    """vgx_tsdf_integrate_depth_image on `L`; returns a Frame (counts: the five of vgx_projective_counts)"""
    out = Frame()
    out.counts = dict(n_candidate_blocks=0, n_new_blocks=0, n_updates=0, n_carved=0, n_cleared=0)
    out.branch = np.zeros((0,), np.int8)
    out.dropped_off = np.zeros((0,), bool)
    if img.width * img.height == 0:
        return out
    code, lo, hi = box(img.width, img.height, cam, cfg, T, L.voxel_size, L.vps)
    assert code == OK, code
    vps, vs = L.vps, F(L.voxel_size)
    T = np.asarray(T, F)
    nx, ny, nz = (hi - lo + 1).tolist()
    out.counts["n_candidate_blocks"] = nx * ny * nz
    # candidates in ascending (z, y, x); the voxels of a block in its storage order lx + vps (ly + vps lz)
    bz, by, bx = np.meshgrid(np.arange(nz) + lo[2], np.arange(ny) + lo[1], np.arange(nx) + lo[0], indexing="ij")
    blocks = np.stack([bx.ravel(), by.ravel(), bz.ravel()], 1).astype(np.int64)
    lz, ly, lx = np.meshgrid(np.arange(vps), np.arange(vps), np.arange(vps), indexing="ij")
    local = np.stack([lx.ravel(), ly.ravel(), lz.ravel()], 1)
    v = blocks[:, None, :] * vps + local[None, :, :]                      # [blocks][vpb][3]
    g = (v.astype(F) + F(0.5)) * vs
    # into the camera frame
    p = g - T[4:]
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    qw, qx, qy, qz = T[0], -T[1], -T[2], -T[3]
    uvx, uvy, uvz = qy * pz - qz * py, qz * px - qx * pz, qx * py - qy * px
    uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
    ccx, ccy, ccz = qy * uvz - qz * uvy, qz * uvx - qx * uvz, qx * uvy - qy * uvx
    x, y, z = (px + qw * uvx) + ccx, (py + qw * uvy) + ccy, (pz + qw * uvz) + ccz
    branch = np.full(z.shape, NO_PIXEL, np.int8)
    with np.errstate(all="ignore"):
        front = z > 0
        ua = ((x / z) * F(cam.fx) + F(cam.cx)) + F(0.5)
        va = ((y / z) * F(cam.fy) + F(cam.cy)) + F(0.5)
        seen = front & (ua >= 0) & (ua < F(img.width)) & (va >= 0) & (va < F(img.height))
        ui = np.where(seen, np.floor(ua), 0).astype(np.int64)
        vi = np.where(seen, np.floor(va), 0).astype(np.int64)
        d = img.z(cam)[vi, ui]
        color = img.rgba()[vi, ui]
        valid = seen & (d > 0) & (d < np.inf) & (d >= F(cam.min_depth_m)) & (d <= F(cam.max_depth_m))
        branch[seen & ~valid] = INVALID_DEPTH
        trunc, max_ray, min_ray = F(cfg.default_truncation_distance), F(cfg.max_ray_length_m), F(cfg.min_ray_length_m)
        r_v = np.sqrt((x * x + y * y) + z * z)
        s = r_v / z
        r_s = d * s
        sdf = (d - z) * s
        short = valid & (r_s < min_ray)
        branch[short] = TOO_SHORT
        rest = valid & ~short
        clearing = rest & (r_s > max_ray)
        clear_ok = clearing & bool(cfg.allow_clear and cfg.voxel_carving_enabled) & (r_v + trunc <= max_ray)
        branch[clearing & ~clear_ok] = CLEAR_REFUSED
        sdf = np.where(clear_ok, max_ray - r_v, sdf)
        rest = rest & ~clearing
        behind = rest & (sdf < -trunc)
        branch[behind] = BEHIND
        rest = rest & ~behind
        carve = rest & (sdf > trunc)
        carve_ok = carve & bool(cfg.voxel_carving_enabled)
        branch[carve & ~carve_ok] = CARVE_REFUSED
        has = (rest & ~carve) | carve_ok | clear_ok
        uw = np.ones_like(d) if cfg.use_const_weight else F(1.0) / (d * d)
        drop = has & bool(cfg.use_weight_dropoff) & (sdf < -vs)
        uw = np.where(drop, np.maximum((uw * (trunc + sdf)) / (trunc - vs), F(0.0)), uw)
        # the voxels as the layer holds them (an absent block: zeros)
        slot = np.array([L.index.get(tuple(b), -1) for b in blocks.tolist()], np.int64)
        held = slot >= 0
        od = np.zeros(z.shape, F)
        ow = np.zeros(z.shape, F)
        oc = np.zeros(z.shape, np.uint32)
        od[held], ow[held], oc[held] = L.distance[slot[held]], L.weight[slot[held]], L.rgba[slot[held]]
        # updateTsdfVoxel
        nw = ow + uw
        changed = has & ~(nw < F(1e-6))
        new_sdf = (sdf * uw + od * ow) / nw
        nd = np.where(new_sdf > 0, np.minimum(trunc, new_sdf), np.maximum(-trunc, new_sdf))
        ncol = np.where(np.abs(sdf) < trunc, blend(oc, color, ow, uw), oc)
        nwc = np.minimum(F(cfg.max_weight), nw)
    branch[has & ~changed] = NO_CHANGE
    branch[changed] = UPDATED
    branch[changed & carve_ok] = CARVED
    branch[changed & clear_ok] = CLEARED
    # blocks: a new one iff a voxel of it changed, slots in candidate order behind the blocks held
    new = ~held & changed.any(1)
    slot[new] = len(L.block_index) + np.arange(int(new.sum()))
    n_new = int(new.sum())
    if n_new:
        vpb = vps ** 3
        L.block_index = np.concatenate([L.block_index, blocks[new].astype(np.int32)])
        L.distance = np.concatenate([L.distance, np.zeros((n_new, vpb), F)])
        L.weight = np.concatenate([L.weight, np.zeros((n_new, vpb), F)])
        L.rgba = np.concatenate([L.rgba, np.zeros((n_new, vpb), np.uint32)])
        for b, s_ in zip(blocks[new].tolist(), slot[new].tolist()):
            L.index[tuple(b)] = s_
    rows, cols = np.nonzero(changed)
    L.distance[slot[rows], cols] = nd[rows, cols]
    L.weight[slot[rows], cols] = nwc[rows, cols]
    L.rgba[slot[rows], cols] = ncol[rows, cols]
    out.counts.update(n_new_blocks=n_new, n_updates=int(changed.sum()), n_carved=int((changed & carve_ok).sum()),
                      n_cleared=int((changed & clear_ok).sum()))
    out.branch, out.dropped_off, out.new_blocks, out.held_blocks = branch, drop & changed, n_new, int((held & changed.any(1)).sum())
    out.sdf, out.weight, out.voxel = sdf, uw, v
    return out
