/*
 * A driver for the one ORBmatcher entry point oracle/ref_matcher/harness.cpp has none for:
 *   int ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
 * AUTHORING ONLY (tools/ref_matcher_scw_goldens.py compiles it into oracle/_ref/, against libref_matcher.so, which already holds the whole of the
 * reference's ORBmatcher.cpp and the stand-in KeyFrame / MapPoint members of harness.cpp).  All of this file is the project's own text: it builds
 * one KeyFrame and the MapPoints from flat arrays through the public members of the stand-in headers of oracle/ref_matcher/, pre-fills vpMatched,
 * hands the reference a vpPoints that still holds the bad and the already-found points - so that its own skips run - calls the overload and
 * returns vpMatched as ids.  The harness's probe log cannot be switched on from here, so outputs are all there is to store.
 */
#include "MapPoint.h"
#include "KeyFrame.h"
#include "Frame.h"
#include "ORBmatcher.h"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace Jetson_SLAM;

namespace {

cv::Mat floats(const float *p, int rows, int cols)
{
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.at<float>(r, c) = p[r * cols + c];
    return m;
}

cv::Mat bytes32(const uint8_t *d, int n)
{
    cv::Mat m(n > 0 ? n : 1, 32, CV_8U);
    if (n > 0) std::memcpy(m.data, d, (size_t)n * 32);
    return m;
}

}  // namespace

extern "C" {

int rm_scw_abi_version(void) { return 1; }

/*
 * The keyframe: N keypoints (kx, ky, octave, kf_desc) with the grid CSR the caller built (cell (i, j) at i * rows + j), camera = fx fy cx cy,
 * bounds = mnMinX mnMaxX mnMinY mnMaxY, inv = the two grid element inverses, the scale table and mfLogScaleFactor.  The point table: n_pts
 * points (pos and normal n_pts x 3, mfMaxDistance, mfMinDistance, descriptor, bad).  vpPoints = list[0 .. n_list) (ids into the table);
 * vpMatched[k] = the point matched_in[k], or NULL at -1.  Returns the reference's return value; matched_out[k] = the id in vpMatched[k] or -1.
 */
int rm_scw_search(int N, const float *kx, const float *ky, const int32_t *octave, const uint8_t *kf_desc, int cols, int rows, const int32_t *cell_start,
                  const int32_t *cell_items, const float *camera, const float *bounds, const float *inv, int n_levels, const float *scale,
                  float log_scale, const float *Scw, int n_pts, const float *pos, const float *normal, const float *maxd, const float *mind,
                  const uint8_t *desc, const uint8_t *bad, int n_list, const int32_t *list, const int32_t *matched_in, int th, int32_t *matched_out)
{
    KeyFrame kf;
    kf.mnId = 0;
    kf.N = N;
    kf.mvKeysUn.resize((size_t)N);
    for (int k = 0; k < N; k++) {
        kf.mvKeysUn[k].pt.x = kx[k];
        kf.mvKeysUn[k].pt.y = ky[k];
        kf.mvKeysUn[k].octave = octave[k];
    }
    kf.mvuRight.assign((size_t)N, -1.0f);
    kf.mDescriptors = bytes32(kf_desc, N);
    kf.mvpMapPoints.assign((size_t)N, nullptr);
    kf.mnGridCols = cols;
    kf.mnGridRows = rows;
    kf.mfGridElementWidthInv = inv[0];
    kf.mfGridElementHeightInv = inv[1];
    kf.mGrid.assign((size_t)cols, std::vector<std::vector<size_t> >((size_t)rows));
    for (int i = 0; i < cols; i++)
        for (int j = 0; j < rows; j++)
            for (int p = cell_start[i * rows + j]; p < cell_start[i * rows + j + 1]; p++) kf.mGrid[i][j].push_back((size_t)cell_items[p]);
    kf.fx = camera[0], kf.fy = camera[1], kf.cx = camera[2], kf.cy = camera[3];
    kf.mnMinX = bounds[0], kf.mnMaxX = bounds[1], kf.mnMinY = bounds[2], kf.mnMaxY = bounds[3];
    kf.mnScaleLevels = n_levels;
    kf.mfLogScaleFactor = log_scale;
    kf.mvScaleFactors.assign(scale, scale + n_levels);

    std::vector<MapPoint> table((size_t)(n_pts > 0 ? n_pts : 0));
    for (int i = 0; i < n_pts; i++) {
        MapPoint &p = table[(size_t)i];
        p.mnId = (long unsigned)i;
        p.nObs = 1;
        p.mbBad = bad[i] != 0;
        p.mpReplaced = nullptr;
        p.mWorldPos = floats(pos + 3 * (size_t)i, 3, 1);
        p.mNormalVector = floats(normal + 3 * (size_t)i, 3, 1);
        p.mDescriptor = bytes32(desc + 32 * (size_t)i, 1);
        p.mfMaxDistance = maxd[i];
        p.mfMinDistance = mind[i];
    }
    std::vector<MapPoint *> vpPoints((size_t)n_list), vpMatched((size_t)N, nullptr);
    for (int i = 0; i < n_list; i++) vpPoints[(size_t)i] = &table[(size_t)list[i]];
    for (int k = 0; k < N; k++)
        if (matched_in[k] >= 0) vpMatched[(size_t)k] = &table[(size_t)matched_in[k]];

    ORBmatcher matcher(0.75f, true);                 /* LoopClosing::ComputeSim3's (LoopClosing.cpp:241) */
    const int found = matcher.SearchByProjection(&kf, floats(Scw, 4, 4), vpPoints, vpMatched, th);
    for (int k = 0; k < N; k++) matched_out[k] = vpMatched[(size_t)k] ? (int32_t)vpMatched[(size_t)k]->mnId : -1;
    return found;
}

}  /* extern "C" */
