// k_frame.hip - the host-side unpacking the reference's Frame constructor does after the front-end, moved to the device
// (SURVEY.md 8f row n4):
//   Frame.cpp:119-196  four blocking SyncedMem::to_cpu() + a host loop turning the keypoint SoA into cv::KeyPoint records
//                      -> k_unpack_keypoints: one AoS record (the memory layout of cv::KeyPoint) per keypoint, so the frame comes
//                         back with one copy for the keypoints and one for the descriptors
//   Frame.cpp:463-479, 696-706  AssignFeaturesToGrid / PosInGrid: per keypoint of mvKeysUn cell = (round((x - minX) * invW),
//                      round((y - minY) * invH)), appended to mGrid[cx][cy] in keypoint order
//                      -> k_assign_grid: CSR over cols x rows cells (cell (i, j) at i*rows + j like mGrid[i][j]), items of a cell in
//                         ascending keypoint order (the reference's push_back order); with a camera the undistorted coordinates of k_undistort
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

__global__ __launch_bounds__(256) void k_unpack_keypoints(const int32_t *__restrict__ soa, int n, jsorb_keypoint *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    jsorb_keypoint k;
    k.x = (float)soa[i];                                    // mvKeys[i].pt.x = kp_x[i]  (int -> float)
    k.y = (float)soa[n + i];
    k.response = (float)soa[2 * (size_t)n + i];
    k.angle = __int_as_float(soa[3 * (size_t)n + i]);       // the angle block holds float bits
    k.octave = soa[4 * (size_t)n + i];
    k.size = (float)soa[5 * (size_t)n + i];
    k.class_id = -1;                                        // cv::KeyPoint default
    out[i] = k;
}

// one workgroup: assign_grid_csr (k_search_common.h)
__global__ __launch_bounds__(1024) void k_assign_grid(const int32_t *__restrict__ soa, const float *__restrict__ xy_un, int n, float min_x, float min_y, float inv_w, float inv_h,
                                                       int cols, int rows, int32_t *__restrict__ cell_start, int32_t *__restrict__ cell_items)
{
    extern __shared__ int s_grid[];          // [n_cells] counts -> starts, [n_cells] cursors, [1024] scan scratch
    assign_grid_csr(n, cols * rows, s_grid, cell_start, cell_items, [&](int i) -> int {
        const float x = xy_un ? xy_un[i] : (float)soa[i], y = xy_un ? xy_un[n + i] : (float)soa[n + i];      // mvKeysUn (Frame.cpp:468)
        return pos_in_grid(x, y, min_x, min_y, inv_w, inv_h, cols, rows);                                       // PosInGrid; NaN / beyond int: no cell
    });
}

void launch_unpack_keypoints(const int32_t *soa, int n, jsorb_keypoint *out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_unpack_keypoints, dim3((n + 255) / 256), dim3(256), 0, s, soa, n, out);
}

void launch_assign_grid(const int32_t *soa, const float *xy_un, int n, float min_x, float min_y, float inv_w, float inv_h, int cols, int rows,
                        int32_t *cell_start, int32_t *cell_items, hipStream_t s)
{
    const size_t lds = (size_t)(2 * cols * rows + 1024) * sizeof(int);
    hipLaunchKernelGGL(k_assign_grid, dim3(1), dim3(1024), lds, s, soa, xy_un, n, min_x, min_y, inv_w, inv_h, cols, rows, cell_start, cell_items);
}

} // namespace jsorb
