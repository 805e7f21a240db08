"""CPU-side checks of the mono / RGB-D Frame steps (jsorb_set_camera, jsorb_image_bounds, jsorb_rgbd_depth*): the header, the library and the
binding agree; jsorb_image_bounds equals a numpy float64 restatement of cv::undistortPoints (OpenCV 4, default criteria, P = K) bit for bit on
the shipped calibrations; the reference's k1-only test; the new C++ shim overloads type-check against a declaration-only OpenCV double.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Examples/RGB-D/TUM1.yaml, TUM2.yaml, Examples/Monocular/EuRoC.yaml (fx, fy, cx, cy, k1, k2, p1, p2, k3; k3 = 0 when the yaml has none)
CAMERAS = {
    "tum1": ((517.306408, 516.469215, 318.643040, 255.313989), (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), (640, 480)),
    "tum2": ((520.908620, 521.007327, 325.141442, 249.701764), (0.231222, -0.784899, -0.003257, -0.000105, 0.917205), (640, 480)),
    "euroc_mono": ((458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (752, 480)),
}


@pytest.fixture(scope="module")
def orb():
    import __graft_entry__ as g
    g.build()
    from jetson_slam_amd import orb as _orb
    return _orb


def K_of(intr):
    fx, fy, cx, cy = intr
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def undistort_ref(intr, dist, u, v):
    """cv::undistortPoints(src, dst, K, D, noArray(), K), OpenCV 4 default criteria (5 iterations), in float64 element-wise numpy (no fusion),
    term for term as include/jsorb.h states it.  Returns (x_un, y_un, exits) as float32, float32 and the mask of the icdist < 0 exit."""
    fx, fy, cx, cy = (np.float64(np.float32(a)) for a in intr)
    k1, k2, p1, p2, k3 = (np.float64(np.float32(a)) for a in dist)
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    u = np.asarray(u, np.float32).astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    x, y = (u - cx) * ifx, (v - cy) * ify
    x0, y0 = x.copy(), y.copy()
    done = np.zeros(u.shape, bool)
    exits = np.zeros(u.shape, bool)
    for _ in range(5):
        r2 = x * x + y * y
        with np.errstate(divide="ignore"):
            icdist = np.float64(1.0) / (np.float64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2)
        ex = ~done & (icdist < 0)
        x = np.where(ex, (u - cx) * ifx, x)
        y = np.where(ex, (v - cy) * ify, y)
        exits |= ex
        done |= ex
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(done, x, (x0 - dx) * icdist)
        y = np.where(done, y, (y0 - dy) * icdist)
    return (fx * x + cx).astype(np.float32), (fy * y + cy).astype(np.float32), exits


def bounds_ref(intr, dist, w, h):
    if np.float32(dist[0]) == 0:
        return np.array([0, w, 0, h], np.float32)
    ux, uy, _ = undistort_ref(intr, dist, np.array([0, w, 0, w], np.float32), np.array([0, 0, h, h], np.float32))
    return np.array([min(ux[0], ux[2]), max(ux[1], ux[3]), min(uy[0], uy[1]), max(uy[2], uy[3])], np.float32)


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_image_bounds_match_the_restatement_bit_for_bit(orb, name):
    intr, dist, (w, h) = CAMERAS[name]
    got = orb.image_bounds(K_of(intr), dist, w, h)
    want = bounds_ref(intr, dist, w, h)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert got[0] != 0 and got[1] != w          # a distorted camera: the bounds move
    # the 4-coefficient form (no k3) is the same as k3 = 0
    if dist[4] == 0:
        assert np.array_equal(orb.image_bounds(K_of(intr), dist[:4], w, h), got)


def test_image_bounds_follow_the_k1_only_test(orb):
    intr, dist, (w, h) = CAMERAS["tum1"]
    for d in ((0.0, -0.95, -0.005, 0.0026, 1.16), (0.0, 0.0, 0.01, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, 0.5)):
        got = orb.image_bounds(K_of(intr), d, w, h)
        assert got.tolist() == [0.0, float(w), 0.0, float(h)]


def test_image_bounds_through_the_negative_icdist_exit(orb):
    """a strongly negative k1 sends image corners through OpenCV's icdist < 0 exit (the un-iterated point); jsorb_image_bounds takes the same
    exit there.  The off-centre camera mixes exiting and iterated corners.  (The device side: tests/test_gpu_undistort.py)"""
    intr, _, (w, h) = CAMERAS["tum1"]
    off_centre = (intr[0], intr[1], 40.0, 30.0)
    for ii, dist in ((intr, (-0.5, 0.0, 0.0, 0.0, 0.0)), (intr, (-1.5, 0.0, 0.002, -0.001, 0.0)), (off_centre, (-0.5, 0.0, 0.001, 0.0, 0.0))):
        _, _, exits = undistort_ref(ii, dist, np.array([0, w, 0, w], np.float32), np.array([0, 0, h, h], np.float32))
        assert exits.any()
        got = orb.image_bounds(K_of(ii), dist, w, h)
        want = bounds_ref(ii, dist, w, h)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dist, got, want)
    _, _, exits = undistort_ref(off_centre, (-0.5, 0.0, 0.001, 0.0, 0.0), np.array([0, w, 0, w], np.float32), np.array([0, 0, h, h], np.float32))
    assert not exits.all()


def test_image_bounds_rejects_bad_arguments(orb):
    lib = orb.load_library()
    out = np.zeros(4, np.float32)
    assert lib.jsorb_image_bounds(None, 640, 480, out.ctypes.data) != 0
    cam = orb.make_camera(K_of(CAMERAS["tum1"][0]), CAMERAS["tum1"][1])
    assert lib.jsorb_image_bounds(ctypes.byref(cam), 0, 480, out.ctypes.data) != 0


def test_header_library_and_binding_agree_on_the_new_entry_points(orb):
    names = ("jsorb_set_camera", "jsorb_camera_enabled", "jsorb_image_bounds", "jsorb_keypoints_un_device", "jsorb_copy_keypoints_un",
             "jsorb_unpack_frame_un", "jsorb_rgbd_depth", "jsorb_rgbd_depth_batch_device_async", "jsorb_rgbd_uright_device", "jsorb_rgbd_depth_device",
             "jsorb_copy_rgbd")
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    raw = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in names:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr), n
    assert "typedef struct jsorb_camera { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } jsorb_camera;" in hdr
    assert re.search(r"#define JSORB_DEPTH_F32 0\b", hdr) and re.search(r"#define JSORB_DEPTH_U16 1\b", hdr)
    assert (orb.DEPTH_F32, orb.DEPTH_U16) == (0, 1)
    # kernel-timing ids after the pipeline's, which stay as they were
    assert "JSORB_K_NMS_MS, JSORB_K_RECTIFY, JSORB_K_COUNT }" in hdr
    assert "enum { JSORB_K_UNDISTORT = JSORB_K_COUNT, JSORB_K_RGBD, JSORB_K_COUNT_ALL };" in hdr
    lib.jsorb_kernel_name.restype = ctypes.c_char_p
    assert lib.jsorb_kernel_name(orb.K_UNDISTORT) == b"k_undistort" and lib.jsorb_kernel_name(orb.K_RGBD) == b"k_rgbd"
    assert lib.jsorb_kernel_name(orb.K_RGBD + 1) == b"" and len(orb.KERNELS) == 8
    for m in ("set_camera", "clear_camera", "camera_enabled", "keypoints_undistorted", "unpack_frame_undistorted", "rgbd_depth", "rgbd_result",
              "undistort_kernel_time", "rgbd_kernel_time"):
        assert callable(getattr(orb.ORBExtractor, m))
    assert callable(orb.image_bounds)
    # the ABI struct and the binding's mirror have the same size
    assert ctypes.sizeof(orb.JsorbCamera) == 36


def test_null_handle_calls_fail_cleanly(orb):
    lib = orb.load_library()
    assert lib.jsorb_set_camera(None, None) < 0 and lib.jsorb_camera_enabled(None) < 0
    assert lib.jsorb_keypoints_un_device(None, 0) is None and lib.jsorb_rgbd_uright_device(None, 0) is None
    assert lib.jsorb_rgbd_depth(None, None, 0, 0, 1.0, 40.0, None, None) < 0


OPENCV_DOUBLE = r"""
#pragma once
#include <cstddef>
#include <string>
#include <vector>
#define CV_8UC1 0
#define CV_16UC1 2
#define CV_32FC1 5
#define CV_32F 5
namespace cv {
struct MatStep { size_t v; operator size_t() const { return v; } size_t operator[](int) const; };
class Mat {
public:
    Mat();
    Mat(int rows, int cols, int type);
    bool empty() const;
    int type() const;
    size_t total() const;
    bool isContinuous() const;
    template <typename T> T &at(int i);
    template <typename T> const T &at(int i) const;
    template <typename T> const T &at(int r, int c) const;
    unsigned char *ptr(int row = 0);
    const unsigned char *ptr(int row = 0) const;
    unsigned char *data;
    int rows, cols;
    MatStep step;
};
struct Point2f { float x, y; };
class KeyPoint {
public:
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};
} // namespace cv
"""

FRAME_CHECK = r"""
#define JSORB_WITH_OPENCV
#include "jsorb_compat.hpp"
// the RGB-D / mono Frame constructor body (Frame.cpp:251-354) with the reference's member types
struct Frame {
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    cv::Mat mDescriptors, mK, mDistCoef;
    std::vector<float> mvuRight, mvDepth;
    float mbf = 40.f, mnMinX, mnMaxX, mnMinY, mnMaxY;
    std::vector<std::size_t> mGrid[64][48];
    void build(Jetson_SLAM::ORBExtractor &ex, const cv::Mat &imGray, const cv::Mat &imDepth, float mDepthMapFactor) {
        Jetson_SLAM::SetCamera(ex, mK, mDistCoef);
        orb_cuda::SyncedMem<int> kps;
        orb_cuda::SyncedMem<unsigned char> desc;
        ex.extract(imGray, kps, desc);
        Jetson_SLAM::UnpackFrame(ex, mvKeys, mvKeysUn, mDescriptors);
        Jetson_SLAM::ComputeStereoFromRGBD(ex, imDepth, mDepthMapFactor, mbf, mvuRight, mvDepth);
        Jetson_SLAM::ComputeImageBounds(mK, mDistCoef, imGray.cols, imGray.rows, mnMinX, mnMaxX, mnMinY, mnMaxY);
        Jetson_SLAM::AssignFeaturesToGrid(ex, mnMinX, mnMinY, 64.f / (mnMaxX - mnMinX), 48.f / (mnMaxY - mnMinY), mGrid);
    }
};
int main() { return 0; }
"""


def test_shim_camera_overloads_type_check_against_a_declaration_only_double(tmp_path):
    """TYPE-CHECK ONLY (no OpenCV here): the cv::Mat forms of SetCamera / UnpackFrame(mvKeys, mvKeysUn) / ComputeStereoFromRGBD /
    ComputeImageBounds compile against the reference's member types; the committed reduced double (tests/cpp/opencv_double) keeps compiling too."""
    inc = tmp_path / "ocv" / "opencv2"
    inc.mkdir(parents=True)
    (inc / "core.hpp").write_text(OPENCV_DOUBLE)
    (inc / "imgproc.hpp").write_text("#pragma once\n#include \"core.hpp\"\n"
                                     "namespace cv { enum { COLOR_BGR2GRAY = 6 }; void cvtColor(const Mat &src, Mat &dst, int code, int dstCn = 0); }\n")
    (inc / "imgcodecs.hpp").write_text("#pragma once\n#include \"core.hpp\"\nnamespace cv { Mat imread(const std::string &filename, int flags = 1); }\n")
    src = tmp_path / "frame_rgbd_check.cpp"
    src.write_text(FRAME_CHECK)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", str(tmp_path / "ocv"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "opencv_double"), os.path.join(ROOT, "tests", "cpp", "frame_compile_check.cpp")])


def test_rgbd_example_compiles_and_links(orb, tmp_path):
    lib_dir = os.path.join(ROOT, "jetson_slam_amd")
    exe = str(tmp_path / "rgbd_frame")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rgbd_frame.cpp"),
                           "-L", lib_dir, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib_dir, "-o", exe])
    assert os.path.exists(exe)
