// search_for_initialization.cpp - the matching step of Tracking::MonocularInitialization (Tracking.cpp:724-794) through the C++ shim: extract the
// first frame and keep it on the device as mInitialFrame (KeepInitialFrame: its octaves, angles, descriptors and mvbPrevMatched = mvKeysUn), extract
// the second frame, then matcher.SearchForInitialization(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches, windowSize) as ONE call,
// Jetson_SLAM::SearchForInitialization - no copy of either frame's keypoints or descriptors to the host, one copy back of the matches.  What stays on
// the host is the Initializer and the tests against the feature counts around it.
// Usage: search_for_initialization H W L tile th_fast first.raw second.raw out.bin
//   first.raw / second.raw: H*W bytes each
//   out.bin: int32 nmatches, n1, vnMatches12[n1]; float mvbPrevMatched x[n1], y[n1]
// Build: g++ -std=c++17 -I include examples/search_for_initialization.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jsorb_compat.hpp"

#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48

using orb_cuda::SyncedMem;

static bool rd(const char *path, std::vector<unsigned char> &im)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(im.data(), 1, im.size(), f) == im.size();
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: %s H W L tile th_fast first.raw second.raw out.bin\n", argv[0]); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th_fast = atoi(argv[5]);
    std::vector<unsigned char> first((size_t)H * W), second((size_t)H * W);
    if (!rd(argv[6], first) || !rd(argv[7], second)) { fprintf(stderr, "cannot read the images\n"); return 2; }
    try {
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, L, 9, 14, 7, th_fast, std::string(), tile, tile, false, false, false, true);
        SyncedMem<int> keys;
        SyncedMem<unsigned char> desc;
        ex.extract(first.data(), W, keys, desc);                 // mInitialFrame = Frame(mCurrentFrame), Tracking.cpp:733
        const int n1 = Jetson_SLAM::KeepInitialFrame(ex);        // mvbPrevMatched[i] = mCurrentFrame.mvKeysUn[i].pt, Tracking.cpp:735-737
        if (n1 <= 50) { fprintf(stderr, "too few keypoints to initialise: %d\n", n1); return 3; }       // np_min, Tracking.cpp:731
        ex.extract(second.data(), W, keys, desc);                // the next frame
        // Frame::ComputeImageBounds without distortion (Frame.cpp:772-777) and the grid constants of Frame.cpp:60-61
        const float mnMinX = 0.0f, mnMaxX = (float)W, mnMinY = 0.0f, mnMaxY = (float)H;
        jsorb_init_params prm{};
        prm.window = 50.0f; prm.nn_ratio = 0.9f; prm.th_low = 50; prm.check_orientation = 1;      // ORBmatcher matcher(0.9, true), windowSize 50
        prm.min_x = mnMinX; prm.min_y = mnMinY;
        prm.inv_w = (float)FRAME_GRID_COLS / (mnMaxX - mnMinX); prm.inv_h = (float)FRAME_GRID_ROWS / (mnMaxY - mnMinY);
        prm.cols = FRAME_GRID_COLS; prm.rows = FRAME_GRID_ROWS;
        std::vector<int> mvIniMatches;
        std::vector<float> mvbPrevMatched;
        const int nmatches = Jetson_SLAM::SearchForInitialization(ex, prm, mvIniMatches, &mvbPrevMatched);
        FILE *out = fopen(argv[8], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[8]); return 2; }
        fwrite(&nmatches, 4, 1, out);
        fwrite(&n1, 4, 1, out);
        fwrite(mvIniMatches.data(), 4, mvIniMatches.size(), out);
        fwrite(mvbPrevMatched.data(), 4, mvbPrevMatched.size(), out);
        fclose(out);
        printf("ok n1=%d nmatches=%d\n", n1, nmatches);
        if (nmatches < 50) Jetson_SLAM::DropInitialFrame(ex);    // Tracking.cpp:765-770: too few correspondences, the Initializer is dropped
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
