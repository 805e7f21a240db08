// k_undistort.hip - the per-keypoint host loops of the mono / RGB-D Frame constructors (Frame.cpp:251-354, 357-462), moved to the device:
//   Frame.cpp:718-748  UndistortKeyPoints: cv::undistortPoints over the N keypoints -> mvKeysUn
//                      -> k_undistort: undistort_point (undistort.h) per keypoint of every image of a lane, x_un[N] y_un[N] per image
//   Frame.cpp:996-1017 ComputeStereoFromRGBD: one depth read per keypoint at the DISTORTED position -> mvDepth, mvuRight = kpU.x - mbf/d
//                      -> k_rgbd, with Tracking.cpp:333-334's imDepth.convertTo(CV_32F, mDepthMapFactor) applied to the sampled pixel only
// Both read the compacted keypoint SoA and the per-image counts on the device (no host round trip); one thread per keypoint slot, grid
// (T / 256, images): threads beyond the image's N return at once.
#include "jsorb_launch.h"

namespace jsorb {

__global__ __launch_bounds__(256) void k_undistort(UndistortCam cam, const int32_t *__restrict__ soa, const int *__restrict__ counts, int T,
                                                    float *__restrict__ un, float *__restrict__ un_host)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = counts[b * (JSORB_MAX_LEVELS + 1) + JSORB_MAX_LEVELS];
    if (i >= n) return;
    const int32_t *s = soa + (size_t)b * 6 * T;
    float x, y;
    undistort_point(cam, (float)s[i], (float)s[n + i], &x, &y);      // mat.at<float>(i, 0) = mvKeys[i].pt.x (int -> float, exact)
    float *o = un + (size_t)b * 2 * T;
    o[i] = x;
    o[n + i] = y;
    if (un_host) { un_host[i] = x; un_host[n + i] = y; }           // single image: the pinned host mirror as well
}

__global__ __launch_bounds__(256) void k_rgbd(const int32_t *__restrict__ soa, const int *__restrict__ counts, int T, const float *__restrict__ un,
                                               const uint8_t *__restrict__ depth, size_t image_stride, size_t step, int W, int H, RgbdArgs a,
                                               float *__restrict__ u_out, float *__restrict__ d_out, float *__restrict__ u_host, float *__restrict__ d_host)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = counts[b * (JSORB_MAX_LEVELS + 1) + JSORB_MAX_LEVELS];
    if (i >= n) return;
    const int32_t *s = soa + (size_t)b * 6 * T;
    const int x = s[i], y = s[n + i];
    float d = -1.0f;
    if (x >= 0 && x < W && y >= 0 && y < H) {          // (always true for the extractor's keypoints; keeps the read inside the image)
        const uint8_t *row = depth + (size_t)b * image_stride + (size_t)y * step;
        if (a.format == JSORB_DEPTH_U16) d = (float)reinterpret_cast<const uint16_t *>(row)[x] * a.factor;       // convertTo(CV_32F, factor): one rounding
        else {
            const float raw = reinterpret_cast<const float *>(row)[x];
            d = a.scale ? raw * a.factor : raw;
        }
    }
    float du = -1.0f, dd = -1.0f;
    if (d > 0) {                                        // NaN fails the test, +inf passes (uRight = x - 0)
        const float xu = un ? un[(size_t)b * 2 * T + i] : (float)x;      // kpU.pt.x: mvKeysUn[i] (== mvKeys[i] without a camera)
        dd = d;
        du = xu - a.mbf / d;
    }
    u_out[(size_t)b * T + i] = du;
    d_out[(size_t)b * T + i] = dd;
    if (u_host) { u_host[i] = du; d_host[i] = dd; }
}

void launch_undistort(const UndistortCam &cam, const int32_t *soa, const int *counts, int T, float *un, float *un_host, int n_images, hipStream_t s)
{
    if (n_images <= 0 || T <= 0) return;
    hipLaunchKernelGGL(k_undistort, dim3((T + 255) / 256, n_images), dim3(256), 0, s, cam, soa, counts, T, un, un_host);
}

void launch_rgbd(const int32_t *soa, const int *counts, int T, const float *un, const uint8_t *depth, size_t image_stride, size_t step, int W, int H,
                 const RgbdArgs &a, float *u_out, float *d_out, float *u_host, float *d_host, int n_images, hipStream_t s)
{
    if (n_images <= 0 || T <= 0) return;
    hipLaunchKernelGGL(k_rgbd, dim3((T + 255) / 256, n_images), dim3(256), 0, s, soa, counts, T, un, depth, image_stride, step, W, H, a, u_out, d_out,
                       u_host, d_host);
}

} // namespace jsorb
