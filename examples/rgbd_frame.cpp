// rgbd_frame.cpp - the RGB-D Frame constructor (Frame.cpp:251-354) through the C++ shim: Tracking's camera set once per extractor
// (Jetson_SLAM::SetCamera), then per frame extract -> UnpackFrame (mvKeys, mvKeysUn, descriptors) -> ComputeStereoFromRGBD on the RAW 16-bit
// depth image (the PNG as read: Tracking.cpp:333-334's whole-image conversion is replaced by the per-keypoint one) -> ComputeImageBounds ->
// AssignFeaturesToGrid over mvKeysUn.  No host loop over the keypoints is left.
// Usage: rgbd_frame H W L tile th gray.raw depth.u16 fx fy cx cy k1 k2 p1 p2 k3 bf depth_factor frames out.bin
//   gray.raw: H*W bytes; depth.u16: H*W uint16; depth_factor: the yaml's DepthMapFactor (inverted here as Tracking.cpp:230-234 does)
// out.bin: int32 N, then mvKeys[N] and mvKeysUn[N] (28-byte cv::KeyPoint records), descriptors[32N], mvuRight[N], mvDepth[N] (float32),
//          bounds[4] (float32 minX maxX minY maxY), grid cell starts[64*48+1] and items (int32) of the LAST frame (every frame repeats the same
//          input: the results must not change from frame to frame - checked here).
// Build: g++ -std=c++17 -I include examples/rgbd_frame.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jsorb_compat.hpp"

#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48

template <typename T>
static std::vector<T> read_file(const char *path, size_t n)
{
    std::vector<T> v(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

struct FrameOut {
    std::vector<jsorb_keypoint> mvKeys, mvKeysUn;
    std::vector<unsigned char> mDescriptors;
    std::vector<float> mvuRight, mvDepth;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    std::vector<int32_t> start, items;
};

int main(int argc, char **argv)
{
    if (argc != 21) {
        fprintf(stderr, "usage: %s H W L tile th gray.raw depth.u16 fx fy cx cy k1 k2 p1 p2 k3 bf depth_factor frames out.bin\n", argv[0]);
        return 2;
    }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th = atoi(argv[5]), frames = atoi(argv[19]);
    const size_t n_px = (size_t)H * W;
    auto gray = read_file<unsigned char>(argv[6], n_px);
    auto depth = read_file<uint16_t>(argv[7], n_px);
    jsorb_camera cam;
    float *c = &cam.fx;
    for (int i = 0; i < 9; i++) c[i] = (float)atof(argv[8 + i]);      // fx fy cx cy k1 k2 p1 p2 k3, as Tracking.cpp:80-91 reads them (float)
    const float mbf = (float)atof(argv[17]);
    float mDepthMapFactor = (float)atof(argv[18]);                     // Tracking.cpp:230-234
    if (std::fabs(mDepthMapFactor) < 1e-5) mDepthMapFactor = 1;
    else mDepthMapFactor = 1.0f / mDepthMapFactor;
    try {
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, L, 9, 14, 7, th, "", tile, tile, false, false, false, true);
        Jetson_SLAM::SetCamera(ex, cam);
        FrameOut first, f;
        for (int it = 0; it < frames; it++) {
            orb_cuda::SyncedMem<int> kps;
            orb_cuda::SyncedMem<unsigned char> desc;
            ex.extract(gray.data(), W, kps, desc);                                                         // Frame.cpp:283 ExtractORB
            Jetson_SLAM::UnpackFrame(ex, f.mvKeys, f.mvKeysUn, f.mDescriptors);                             // :285-297, UndistortKeyPoints :299
            Jetson_SLAM::ComputeStereoFromRGBD(ex, depth.data(), JSORB_DEPTH_U16, (size_t)W * 2, mDepthMapFactor, mbf, f.mvuRight, f.mvDepth);   // :301
            Jetson_SLAM::ComputeImageBounds(cam, W, H, f.mnMinX, f.mnMaxX, f.mnMinY, f.mnMaxY);             // :311 (first frame only in the reference)
            std::vector<std::size_t> grid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
            Jetson_SLAM::AssignFeaturesToGrid(ex, f.mnMinX, f.mnMinY, FRAME_GRID_COLS / (f.mnMaxX - f.mnMinX), FRAME_GRID_ROWS / (f.mnMaxY - f.mnMinY), grid);
            f.start.assign(1, 0);
            f.items.clear();
            for (int i = 0; i < FRAME_GRID_COLS; i++)
                for (int j = 0; j < FRAME_GRID_ROWS; j++) {
                    for (std::size_t k : grid[i][j]) f.items.push_back((int32_t)k);
                    f.start.push_back((int32_t)f.items.size());
                }
            if (it == 0) first = f;
            else if (memcmp(first.mvKeysUn.data(), f.mvKeysUn.data(), f.mvKeysUn.size() * sizeof(jsorb_keypoint)) != 0 || first.mvDepth != f.mvDepth ||
                     first.items != f.items || first.mvKeys.size() != f.mvKeys.size()) {
                fprintf(stderr, "frame %d differs from frame 0\n", it);
                return 1;
            }
        }
        FILE *o = fopen(argv[20], "wb");
        if (!o) return 2;
        const int32_t N = (int32_t)f.mvKeys.size();
        fwrite(&N, 4, 1, o);
        fwrite(f.mvKeys.data(), sizeof(jsorb_keypoint), N, o);
        fwrite(f.mvKeysUn.data(), sizeof(jsorb_keypoint), N, o);
        fwrite(f.mDescriptors.data(), 1, (size_t)32 * N, o);
        fwrite(f.mvuRight.data(), 4, N, o);
        fwrite(f.mvDepth.data(), 4, N, o);
        const float b[4] = {f.mnMinX, f.mnMaxX, f.mnMinY, f.mnMaxY};
        fwrite(b, 4, 4, o);
        fwrite(f.start.data(), 4, f.start.size(), o);
        fwrite(f.items.data(), 4, f.items.size(), o);
        fclose(o);
        printf("rgbd_frame: N=%d with depth=%d, bounds %.3f %.3f %.3f %.3f\n", N, (int)std::count_if(f.mvDepth.begin(), f.mvDepth.end(), [](float d) { return d > 0; }),
               b[0], b[1], b[2], b[3]);
    } catch (const std::exception &e) {
        fprintf(stderr, "rgbd_frame: %s\n", e.what());
        return 1;
    }
    return 0;
}
