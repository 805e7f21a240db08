// undistort.h - the keypoint undistortion of Frame::UndistortKeyPoints / Frame::ComputeImageBounds (Frame.cpp:718-778): OpenCV 4's
// cv::undistortPoints(src, dst, K, D, noArray(), K) with its default criteria, for the 4 / 5-coefficient model.  ONE __host__ __device__
// routine: k_undistort (k_undistort.hip) runs it per keypoint, jsorb_image_bounds (jsorb_frame.hip) on the host for the four corners, so the
// two cannot drift apart.  The library builds with -ffp-contract=off -fno-fast-math: every operation below is one IEEE double operation,
// `/` is the correctly rounded division on both sides, nothing is fused.
#pragma once

#include <hip/hip_runtime.h>

namespace jsorb {

// The camera as Tracking.cpp:80-91 reads it: mK (CV_32F, zero skew) and mDistCoef (CV_32F, k3 = 0 in the 4-coefficient form).
struct UndistortCam { float fx, fy, cx, cy, k1, k2, p1, p2, k3; };

// OpenCV 4.x, modules/calib3d/src/undistort.dispatch.cpp, cvUndistortPointsInternal, with R = noArray() and P = K:
//   * cameraMatrix and distCoeffs are converted to double; k[5..11] (rational and thin-prism terms) are 0, tau = 0 -> invMatTilt = I.
//   * criteria = TermCriteria(COUNT, 5, 0.01): exactly 5 iterations, the EPS test is never evaluated.
//   * vecUntilt = I * (x, y, 1) and invProj = 1./1 = 1 give x0 = x, y0 = y.
//   * icdist = (1 + ((k[7]*r2 + k[6])*r2 + k[5])*r2) / (1 + ((k[4]*r2 + k[1])*r2 + k[0])*r2): the numerator is 1 + 0 = 1 exactly.
//   * deltaX = 2*k[2]*x*y + k[3]*(r2 + 2*x*x) + k[8]*r2 + k[9]*r2*r2: the two trailing terms are +0 for finite input and adding +0
//     leaves every nonzero value unchanged (likewise deltaY with k[10], k[11]).
//   * RR = P * R = K * I = K exactly, so xx = (fx*x + 0*y) + cx = fx*x + cx, yy = (0*x + fy*y) + cy = fy*y + cy, ww = 1./(0*x + 0*y + 1) = 1.
// The zero terms can only flip the sign of an exact zero, which the final `+ cx` / `+ cy` erases whenever cx, cy != 0: for finite input the
// expressions below are OpenCV's bit for bit.  (Parity against a live cv::undistortPoints is not pinned by a test: no OpenCV here.)
__host__ __device__ inline void undistort_point(const UndistortCam &c, float px, float py, float *ox, float *oy)
{
    const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
    const double k1 = c.k1, k2 = c.k2, p1 = c.p1, p2 = c.p2, k3 = c.k3;
    const double ifx = 1. / fx, ify = 1. / fy;
    const double u = px, v = py;
    double x = (u - cx) * ifx, y = (v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1. / (1. + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0) {          // OpenCV's regression_14583 exit: the un-iterated normalised point
            x = (u - cx) * ifx;
            y = (v - cy) * ify;
            break;
        }
        const double deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    *ox = (float)(fx * x + cx);
    *oy = (float)(fy * y + cy);
}

// Frame::UndistortKeyPoints tests mDistCoef.at<float>(0) == 0.0, i.e. k1 ALONE: with k1 == 0 mvKeysUn = mvKeys whatever p1, p2, k3 are.
__host__ __device__ inline bool camera_active(const UndistortCam &c) { return c.k1 != 0.0f; }

} // namespace jsorb
