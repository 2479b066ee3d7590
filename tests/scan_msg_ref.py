"""numpy restatement of the scan decode (include/voxgraph_amd.h, "Scans"): what pcl::fromROSMsg + voxblox::convertPointcloud
make of a sensor_msgs/PointCloud2 [recalled: PCL and voxblox_ros are not vendored].  Written from the rules in the header,
not from the kernel: addresses from row_step / point_step, little-endian fields assembled byte by byte, the finite
filter on bit patterns, PCL's packed 0xAARRGGBB, voxblox's grayColorMap."""
import numpy as np

F = np.float32
COLOR_NONE, COLOR_RGB, COLOR_INTENSITY = 0, 1, 2


def field_u32(data, base, offset):
    """the little-endian 32-bit field at base + offset of every point (data: uint8 array, base: int64 array)"""
    at = base + np.int64(offset)
    b = [data[at + k].astype(np.uint32) for k in range(4)]
    return b[0] | (b[1] << np.uint32(8)) | (b[2] << np.uint32(16)) | (b[3] << np.uint32(24))


def gray(v, vmin, vmax):
    """GrayscaleColorMap::colorLookup [recalled]: std::min(max, std::max(min, v)) with their argument order (NaN -> min),
    (v - min) / (max - min) in f32, std::round((double)h * 255.0) -- half away from zero, which for h >= 0 is
    floor(x + 0.5); x has at most 32 significant bits, so the sum is exact in f64"""
    v = np.asarray(v, F)
    vmin, vmax = F(vmin), F(vmax)
    with np.errstate(invalid="ignore"):
        v = np.where(vmin < v, v, vmin).astype(F)
        v = np.where(v < vmax, v, vmax).astype(F)
    h = ((v - vmin).astype(F) / F(vmax - vmin)).astype(F)
    return np.floor(h.astype(np.float64) * 255.0 + 0.5).astype(np.uint8)


def decode(msg, intensity_min=0.0, intensity_max=10000.0, constant_rgba=(0, 0, 0, 0)):
    """msg: width, height, point_step, row_step, offset_x / _y / _z, color_kind, color_offset, data (uint8 array).
    Returns (points [n][3] f32, rgba [n][4] u8, kept: the message index i of every kept point, ascending)."""
    data = np.frombuffer(msg.data, np.uint8)
    i = np.arange(msg.width * msg.height, dtype=np.int64)
    if len(i) == 0:
        return np.zeros((0, 3), F), np.zeros((0, 4), np.uint8), i
    base = (i // msg.width) * np.int64(msg.row_step) + (i % msg.width) * np.int64(msg.point_step)
    xyz = np.stack([field_u32(data, base, o) for o in (msg.offset_x, msg.offset_y, msg.offset_z)], 1)
    finite = (xyz & np.uint32(0x7f800000)) != np.uint32(0x7f800000)          # exponent not all ones
    kept = np.flatnonzero(finite.all(1))
    points = np.ascontiguousarray(xyz[kept]).view(F)
    rgba = np.zeros((len(kept), 4), np.uint8)
    if msg.color_kind == COLOR_NONE:
        rgba[:] = np.asarray(constant_rgba, np.uint8)
    elif msg.color_kind == COLOR_RGB:
        at = base[kept] + np.int64(msg.color_offset)
        rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3] = data[at + 2], data[at + 1], data[at], data[at + 3]
    elif msg.color_kind == COLOR_INTENSITY:
        g = gray(field_u32(data, base[kept], msg.color_offset).view(F), intensity_min, intensity_max)
        rgba[:, 0] = rgba[:, 1] = rgba[:, 2] = g
        rgba[:, 3] = 255
    else:
        raise ValueError("unknown color_kind")
    return points, rgba, kept
