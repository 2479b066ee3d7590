// The per-frame host pass a caller of vgx_tsdf_integrate needs without vgx_scan: what pcl::fromROSMsg +
// voxblox::convertPointcloud amount to [recalled], as one plain single-thread loop over the message -- drop the points
// that are not finite, make one colour per kept point, pack both.  The baseline of profiles/scan_msg_bench.py; built by
// it with g++ -O2.  Same rules as include/voxgraph_amd.h ("Scans"); aligned little-endian layouts only.
#include <cmath>
#include <cstdint>
#include <cstring>

extern "C" int64_t host_convert(const uint8_t* data, uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step,
                                uint32_t ox, uint32_t oy, uint32_t oz, int32_t color_kind, uint32_t color_offset, float vmin,
                                float vmax, float* points, uint8_t* rgba) {
  int64_t n = 0;
  for (uint32_t r = 0; r < height; ++r) {
    const uint8_t* p = data + (size_t)r * row_step;
    for (uint32_t c = 0; c < width; ++c, p += point_step) {
      float x, y, z;
      std::memcpy(&x, p + ox, 4);
      std::memcpy(&y, p + oy, 4);
      std::memcpy(&z, p + oz, 4);
      if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) continue;
      points[3 * n + 0] = x;
      points[3 * n + 1] = y;
      points[3 * n + 2] = z;
      uint8_t* out = rgba + 4 * n;
      if (color_kind == 1) {
        out[0] = p[color_offset + 2];
        out[1] = p[color_offset + 1];
        out[2] = p[color_offset + 0];
        out[3] = p[color_offset + 3];
      } else if (color_kind == 2) {
        float v;
        std::memcpy(&v, p + color_offset, 4);
        v = (vmin < v) ? v : vmin;
        v = (v < vmax) ? v : vmax;
        const float h = (v - vmin) / (vmax - vmin);
        out[0] = out[1] = out[2] = (uint8_t)std::round((double)h * 255.0);
        out[3] = 255;
      } else {
        out[0] = out[1] = out[2] = out[3] = 0;
      }
      ++n;
    }
  }
  return n;
}
