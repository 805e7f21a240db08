// k_rectify.hip - level 0 of every image of a lane from the caller's RAW image through a per-handle rectification map, in ONE launch.
//
// Semantics: cv::remap(src, dst, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit gray images in OpenCV's fixed-point form
// (INTER_BITS = 5), which the reference's stereo driver runs on the host before every TrackStereo (Examples/Stereo/stereo_euroc.cpp:106-107
// build the maps, :145-146 remap both images).  For output pixel (x, y) with fixed-point map entry (ix, iy, a = fy << 5 | fx):
//   out = ( sum over dy, dx in {0, 1} of [tap inside the source] * src[iy+dy][ix+dx] * wx[dx] * wy[dy] + 512 ) >> 10,
//   wx = {32 - fx, fx}, wy = {32 - fy, fy}
// Taps outside the source contribute the border value 0.  Integer arithmetic only; no texture filtering (its weight precision is not
// this contract).  The float maps are converted to the fixed-point form once, on the host, by rectify_convert_maps (the single
// implementation of that step, behind jsorb_rectify_convert_maps).
// Layout: one 256-lane workgroup per RECT_TW x RECT_TH output tile, a lane owns 4 adjacent output pixels in each of RECT_RPL rows (one dword
// store per row, as k_pyramid) and reads their 4 map entries with one 16-byte and one 8-byte load.  The source footprint of a tile under a
// rectification map is a slightly warped box; the host computes its bounding box per tile once (rectify_tile_table) and, when it fits
// RECT_LDS_W x RECT_LDS_H bytes, the workgroup stages it in LDS with dword loads and gathers its taps from there.  Tiles whose
// footprint does not fit (arbitrary user maps, e.g. a permutation of the source pixels) gather their taps straight from global memory;
// both forms read the same source bytes, so the output is the same.  All images of a handle share one map: the XCD-aware grid
// (xcd_grid) sends every tile of an image to one XCD, which streams its images through the map in its own L2.
#include <algorithm>
#include <cmath>

#include "jsorb_launch.h"

namespace jsorb {

__global__ __launch_bounds__(256) void k_rectify(RectMap m, const uint8_t *__restrict__ src, unsigned long long src_stride, int src_step,
                                                 uint8_t *__restrict__ dst, unsigned long long dst_stride, int dst_pitch, int W, int H, int n_images)
{
    __shared__ unsigned s_box[RECT_LDS_W / 4 * RECT_LDS_H];
    int b, blk;
    if (!xcd_map(m.ntx * m.nty, n_images, b, blk)) return;
    const int tr = blk / m.ntx, tc = blk - tr * m.ntx;
    // a lane owns 4 pixels in each of RECT_RPL rows, RECT_TH / RECT_RPL apart; their map entries are requested first (they do not depend on the
    // tile's source box), so that their latency overlaps the staging of the box
    const int x = tc * RECT_TW + (threadIdx.x & (RECT_TW / 4 - 1)) * 4, y0 = tr * RECT_TH + threadIdx.x / (RECT_TW / 4);
    int4 xy[RECT_RPL];
    uint2 a2[RECT_RPL];
#pragma unroll
    for (int r = 0; r < RECT_RPL; r++) {
        const int y = y0 + r * (RECT_TH / RECT_RPL);
        if (x < W && y < H) {
            const size_t mo = (size_t)y * m.pitch + x;
            xy[r] = *reinterpret_cast<const int4 *>(m.xy + mo);
            a2[r] = *reinterpret_cast<const uint2 *>(m.a + mo);
        }
    }
    const int4 t = m.tiles[blk];                  // source box of the tile: x0 (multiple of 4), y0, rows, dwords per row staged in LDS (0: global taps)
    const uint8_t *img = src + (unsigned long long)b * src_stride;
    const bool staged = t.w != 0;
    if (staged) {
        const bool al4 = ((reinterpret_cast<unsigned long long>(img) | (unsigned long long)src_step) & 3ull) == 0;
        for (int i = threadIdx.x; i < t.z * (RECT_LDS_W / 4); i += 256) {
            const int c = i & (RECT_LDS_W / 4 - 1);
            if (c >= t.w) continue;
            const int sx = t.x + 4 * c, sy = t.y + i / (RECT_LDS_W / 4);
            const uint8_t *p = img + (long long)sy * src_step + sx;
            unsigned v = 0;
            if (al4 && sx + 3 < W) v = *reinterpret_cast<const unsigned *>(p);
            else
                for (int k = 0; k < 4; k++)
                    if (sx + k < W) v |= (unsigned)p[k] << (8 * k);
            s_box[i] = v;
        }
        __syncthreads();
    }
    const uint8_t *box = reinterpret_cast<const uint8_t *>(s_box);
    auto tap = [&](int sx, int sy) -> int {
        if ((unsigned)sx >= (unsigned)W || (unsigned)sy >= (unsigned)H) return 0;
        if (staged) return box[(sy - t.y) * RECT_LDS_W + (sx - t.x)];
        return img[(long long)sy * src_step + sx];
    };
#pragma unroll
    for (int r = 0; r < RECT_RPL; r++) {
        const int y = y0 + r * (RECT_TH / RECT_RPL);
        if (x >= W || y >= H) break;
        const int ent[4] = {xy[r].x, xy[r].y, xy[r].z, xy[r].w};
        const unsigned av[4] = {a2[r].x & 0xFFFFu, a2[r].x >> 16, a2[r].y & 0xFFFFu, a2[r].y >> 16};
        unsigned out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (x + k >= W) break;
            const int ix = (int)(short)(ent[k] & 0xFFFF), iy = ent[k] >> 16;
            const int fx = av[k] & 31, fy = (av[k] >> 5) & 31;
            const int top = tap(ix, iy) * (32 - fx) + tap(ix + 1, iy) * fx;
            const int bot = tap(ix, iy + 1) * (32 - fx) + tap(ix + 1, iy + 1) * fx;
            out |= (unsigned)((top * (32 - fy) + bot * fy + 512) >> 10) << (8 * k);
        }
        *reinterpret_cast<unsigned *>(dst + (unsigned long long)b * dst_stride + (size_t)y * dst_pitch + x) = out;
    }
}

void launch_rectify(const RectMap &m, const uint8_t *src, size_t src_stride, int src_step, uint8_t *dst, size_t dst_stride, int dst_pitch, int W, int H,
                    int n_images, hipStream_t s)
{
    hipLaunchKernelGGL(k_rectify, xcd_grid(m.ntx * m.nty, n_images), dim3(256), 0, s, m, src, (unsigned long long)src_stride, src_step, dst,
                       (unsigned long long)dst_stride, dst_pitch, W, H, n_images);
}

// OpenCV's float -> fixed-point map conversion (cv::convertMaps to CV_16SC2 + CV_16UC1, as remap does internally): X = round-half-even(mapx * 32)
// (exact in f32); NaN, inf and values whose X does not fit an int give X = INT_MIN (what the SSE conversion returns), i.e. a pixel outside the
// source.  ix = saturate_cast<short>(X >> 5), a = (Y & 31) << 5 | (X & 31).
static inline int fixed_coord(float v)
{
    const float f = v * 32.0f;
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
    return (int)lrintf(f);
}

void rectify_convert_maps(const float *mapx, const float *mapy, size_t n, int16_t *xy, uint16_t *a)
{
    for (size_t i = 0; i < n; i++) {
        const int X = fixed_coord(mapx[i]), Y = fixed_coord(mapy[i]);
        xy[2 * i] = (int16_t)std::min(32767, std::max(-32768, X >> 5));
        xy[2 * i + 1] = (int16_t)std::min(32767, std::max(-32768, Y >> 5));
        a[i] = (uint16_t)(((Y & 31) << 5) | (X & 31));
    }
}

// Per output tile: the bounding box of every source tap inside the image (zero-weight taps included: the kernel reads all four), its left edge
// rounded down to a dword: {x0, y0, rows, dwords per row}.  Staged in LDS when it fits RECT_LDS_W x RECT_LDS_H (dwords per row 0: it does not,
// global taps); a tile with no tap inside the source stages nothing (0 rows).
void rectify_tile_table(const int16_t *xy, const uint16_t *a, int W, int H, int map_pitch, int ntx, int nty, int32_t *tiles)
{
    (void)a;
    for (int tr = 0; tr < nty; tr++)
        for (int tc = 0; tc < ntx; tc++) {
            int x0 = W, y0 = H, x1 = -1, y1 = -1;
            for (int y = tr * RECT_TH; y < std::min(H, (tr + 1) * RECT_TH); y++)
                for (int x = tc * RECT_TW; x < std::min(W, (tc + 1) * RECT_TW); x++) {
                    const int ix = xy[2 * ((size_t)y * map_pitch + x)], iy = xy[2 * ((size_t)y * map_pitch + x) + 1];
                    for (int dy = 0; dy < 2; dy++)
                        for (int dx = 0; dx < 2; dx++) {
                            const int sx = ix + dx, sy = iy + dy;
                            if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
                            x0 = std::min(x0, sx); x1 = std::max(x1, sx);
                            y0 = std::min(y0, sy); y1 = std::max(y1, sy);
                        }
                }
            int32_t *o = tiles + 4 * ((size_t)tr * ntx + tc);
            if (x1 < 0) { o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 1; continue; }
            x0 &= ~3;
            const bool fits = x1 - x0 < RECT_LDS_W && y1 - y0 < RECT_LDS_H;
            o[0] = x0; o[1] = y0; o[2] = y1 - y0 + 1; o[3] = fits ? (x1 - x0) / 4 + 1 : 0;
        }
}

} // namespace jsorb
