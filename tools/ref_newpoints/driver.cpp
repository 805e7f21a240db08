/*
 * tools/ref_newpoints/driver.cpp - a world of tests/new_points_cases.py through the reference's own LocalMapping::CreateNewMapPoints, with its
 * KeyFrame::UnprojectStereo / AddMapPoint and MapPoint's constructor, AddObservation, ComputeDistinctiveDescriptors and UpdateNormalAndDepth:
 * src/LocalMapping.cpp, src/KeyFrame.cpp and src/MapPoint.cpp compiled unmodified against this folder's opencv2/core/core.hpp and the stand-in
 * headers of tools/ref_culling (included by path, unchanged).
 * ORBmatcher::SearchForTriangulation is STUBBED: the two sets of stand-ins (oracle/ref_matcher's fake Mat, this folder's real one) do not combine
 * in one program.  The stub applies exactly the rule of ORBmatcher.cpp:686-690 - a KF1 keypoint with a map point is skipped, at the moment of the
 * call - over the candidates recorded for the world: the matches of every neighbour over the map as it is before the loop, in ascending idx1
 * (vMatchedPairs' order, :800-806).  What LocalMapping.cpp names and this loop never reaches (Optimizer, Fuse, LoopClosing) aborts.
 * Usage: ref_newpoints world.bin out.bin (the layouts: new_points_cases.world_bytes / unpack).
 * The keyframes are laid out in one block in (order_key, slot) order, so that std::map<KeyFrame*, size_t> walks them in that order.
 * AUTHORING TOOLING ONLY.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <thread>
#include <vector>

#define protected public
#define private public
#include "LocalMapping.h"
#include "MapPoint.h"
#include "KeyFrame.h"
#undef protected
#undef private

namespace Jetson_SLAM {
static void unreachable(const char *what) { std::fprintf(stderr, "ref_newpoints: %s was reached\n", what); std::abort(); }
static std::map<KeyFrame *, const int32_t *> g_candidates;      // per neighbour: its recorded match per idx1, -1 none
static int g_n1 = 0;
ORBmatcher::ORBmatcher(float, bool) {}
int ORBmatcher::DescriptorDistance(const cv::Mat &a, const cv::Mat &b)      // ORBmatcher.cpp:2143-2161: the popcount of the xor over 32 bytes
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a.ptr<unsigned char>()[i] ^ b.ptr<unsigned char>()[i]));
    return d;
}
int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, const bool)
{
    const int32_t *cand = g_candidates.at(pKF2);
    vMatchedPairs.clear();
    for (int idx1 = 0; idx1 < g_n1; idx1++) {
        MapPoint *pMP1 = pKF1->GetMapPoint(idx1);
        if (pMP1) continue;                      // :686-690
        if (cand[idx1] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)idx1, (size_t)cand[idx1]));
    }
    return (int)vMatchedPairs.size();
}
int ORBmatcher::Fuse(KeyFrame *, const std::vector<MapPoint *> &, const float) { unreachable("Fuse"); return 0; }
void Optimizer::LocalBundleAdjustment(KeyFrame *, bool *, Map *) { unreachable("LocalBundleAdjustment"); }
void LoopClosing::InsertKeyFrame(KeyFrame *) { unreachable("LoopClosing::InsertKeyFrame"); }
}  // namespace Jetson_SLAM

using namespace Jetson_SLAM;

template <class T> static std::vector<T> take(const unsigned char *&p, size_t n)
{
    std::vector<T> v(n);
    std::memcpy(v.data(), p, n * sizeof(T));
    p += n * sizeof(T);
    return v;
}
static int32_t bits(float f) { int32_t i; std::memcpy(&i, &f, 4); return i; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> raw;
    unsigned char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) raw.insert(raw.end(), buf, buf + n);
    std::fclose(f);
    const unsigned char *p = raw.data();
    const std::vector<int32_t> hd = take<int32_t>(p, 8);
    const int S = hd[0], n_rows = hd[1], pool = hd[2], cur = hd[3], n1 = hd[4], T = hd[5], L = hd[6], kf_id = hd[7];
    const auto state = take<int32_t>(p, S);
    const auto key = take<int64_t>(p, S);
    const auto off = take<int32_t>(p, S), len = take<int32_t>(p, S), pts = take<int32_t>(p, pool), octave = take<int32_t>(p, pool);
    const auto x = take<float>(p, pool), y = take<float>(p, pool), uright = take<float>(p, pool), depth = take<float>(p, pool), raw_x = take<float>(p, pool),
               raw_y = take<float>(p, pool);
    const auto desc = take<unsigned char>(p, (size_t)pool * 32);
    const auto bad = take<int32_t>(p, n_rows), nb = take<int32_t>(p, T), pose_slot = take<int32_t>(p, S);
    const auto poses = take<float>(p, (size_t)(1 + T) * 18);      // Rcw 9, tcw 3, fx fy cx cy mb mbf
    const auto sf = take<float>(p, L), sigma2 = take<float>(p, L), scale = take<float>(p, 1);
    const auto cand = take<int32_t>(p, (size_t)T * n1);

    Map map;
    KeyFrameDatabase db;
    std::vector<int> order;
    for (int s = 0; s < S; s++)
        if (state[s] != 0) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
    KeyFrame *block = static_cast<KeyFrame *>(::operator new(sizeof(KeyFrame) * (order.size() + 1)));
    std::vector<KeyFrame *> kf(S, nullptr);
    std::map<KeyFrame *, int> slot_of;
    std::vector<MapPoint *> point(n_rows, nullptr);
    std::map<MapPoint *, int> row_of;
    Frame none_frame;
    none_frame.mTcw = cv::Mat::eye(4, 4, CV_32F);
    KeyFrame *none = new (block + order.size()) KeyFrame(none_frame, &map, &db);
    for (int r = 0; r < n_rows; r++) {
        point[r] = new MapPoint(cv::Mat::zeros(3, 1, CV_32F), none, &map);
        point[r]->mbBad = bad[r] != 0;
        row_of[point[r]] = r;
    }
    for (size_t i = 0; i < order.size(); i++) {
        const int s = order[i], ps = pose_slot[s];
        Frame fr;
        fr.N = len[s];
        fr.mDescriptors = cv::Mat(len[s] > 0 ? len[s] : 1, 32, CV_8U);
        for (int j = 0; j < len[s]; j++) {
            const int e = off[s] + j, r = pts[e];
            cv::KeyPoint kp;
            kp.octave = octave[e];
            kp.pt.x = x[e]; kp.pt.y = y[e];
            fr.mvKeysUn.push_back(kp);
            kp.pt.x = raw_x[e]; kp.pt.y = raw_y[e];
            fr.mvKeys.push_back(kp);
            fr.mvuRight.push_back(uright[e]);
            fr.mvDepth.push_back(depth[e]);
            fr.mvpMapPoints.push_back(r >= 0 && r < n_rows ? point[r] : nullptr);
            std::memcpy(fr.mDescriptors.ptr<unsigned char>(j), &desc[(size_t)e * 32], 32);
        }
        fr.mTcw = cv::Mat::eye(4, 4, CV_32F);
        fr.mK = cv::Mat::eye(3, 3, CV_32F);
        if (ps >= 0) {
            const float *q = &poses[(size_t)ps * 18];
            for (int a = 0; a < 3; a++) {
                for (int b = 0; b < 3; b++) fr.mTcw.at<float>(a, b) = q[3 * a + b];
                fr.mTcw.at<float>(a, 3) = q[9 + a];
            }
            fr.fx = q[12]; fr.fy = q[13]; fr.cx = q[14]; fr.cy = q[15]; fr.mb = q[16]; fr.mbf = q[17];
            fr.invfx = 1.0f / fr.fx; fr.invfy = 1.0f / fr.fy;
            fr.mK.at<float>(0, 0) = fr.fx; fr.mK.at<float>(1, 1) = fr.fy; fr.mK.at<float>(0, 2) = fr.cx; fr.mK.at<float>(1, 2) = fr.cy;
        }
        fr.mnScaleLevels = L;
        fr.mfScaleFactor = scale[0];
        fr.mvScaleFactors = sf; fr.mvLevelSigma2 = sigma2;
        kf[s] = new (block + i) KeyFrame(fr, &map, &db);
        kf[s]->mnId = s == cur ? (long unsigned)kf_id : 100000 + s;
        kf[s]->mbBad = state[s] != 1;
        slot_of[kf[s]] = s;
    }
    for (int s = 0; s < S; s++)
        if (kf[s] && state[s] == 1)
            for (int j = 0; j < len[s]; j++) {
                const int r = pts[off[s] + j];
                if (r >= 0 && r < n_rows && !bad[r]) point[r]->AddObservation(kf[s], j);
            }
    KeyFrame *current = kf[cur];
    for (int t = 0; t < T; t++) {
        current->mvpOrderedConnectedKeyFrames.push_back(kf[nb[t]]);
        g_candidates[kf[nb[t]]] = &cand[(size_t)t * n1];
    }
    g_n1 = n1;
    // cos(2*atan2(mb/2, mvDepth[i])) of every keypoint, the expression of LocalMapping.cpp:318 with this build's libm: the world's cos_stereo
    std::vector<int32_t> cos_out(pool, bits(1.0f));
    for (int s = 0; s < S; s++)
        if (kf[s])
            for (int j = 0; j < len[s]; j++) {
                const float c = cos(2 * atan2(kf[s]->mb / 2, kf[s]->mvDepth[j]));
                cos_out[off[s] + j] = bits(c);
            }

    LocalMapping mapper(&map, false);
    mapper.mpCurrentKeyFrame = current;
    mapper.CreateNewMapPoints();

    std::vector<int32_t> out;
    out.push_back((int32_t)mapper.mlpRecentAddedMapPoints.size());
    for (MapPoint *mp : mapper.mlpRecentAddedMapPoints) {
        const std::map<KeyFrame *, size_t> obs = mp->GetObservations();
        int idx1 = -1, t = -1, idx2 = -1;
        for (auto &o : obs) {
            if (o.first == current) idx1 = (int)o.second;
            else { idx2 = (int)o.second; for (int i = 0; i < T; i++) if (kf[nb[i]] == o.first) { t = i; break; } }
        }
        out.push_back(idx1); out.push_back(t); out.push_back(idx2);
        out.push_back((int32_t)mp->mnFirstKFid);
        out.push_back(slot_of[mp->GetReferenceKeyFrame()]);
        out.push_back(mp->mnVisible); out.push_back(mp->mnFound);
        const cv::Mat P = mp->GetWorldPos(), N = mp->GetNormal();
        for (int c = 0; c < 3; c++) out.push_back(bits(P.at<float>(c)));
        for (int c = 0; c < 3; c++) out.push_back(bits(N.at<float>(c)));
        out.push_back(bits(mp->mfMaxDistance));
        out.push_back(bits(mp->GetMaxDistanceInvariance()));
        out.push_back(bits(mp->GetMinDistanceInvariance()));
        const cv::Mat d = mp->GetDescriptor();
        for (int w = 0; w < 8; w++) { int32_t v; std::memcpy(&v, d.ptr<unsigned char>() + 4 * w, 4); out.push_back(v); }
        out.push_back(mp->isBad());
    }
    // the pool as the keyframes hold it now: a new point by its creation number behind the table's rows; registered from the observations
    std::map<MapPoint *, int> created;
    int k = 0;
    for (MapPoint *mp : mapper.mlpRecentAddedMapPoints) created[mp] = k++;
    std::vector<int32_t> pool_out(pool, -1), reg_out(pool, 0);
    for (int s = 0; s < S; s++) {
        if (!kf[s]) continue;
        const std::vector<MapPoint *> now = kf[s]->GetMapPointMatches();
        for (int j = 0; j < len[s]; j++) {
            MapPoint *mp = now[j];
            if (!mp) continue;
            pool_out[off[s] + j] = created.count(mp) ? n_rows + created[mp] : row_of[mp];
            const std::map<KeyFrame *, size_t> obs = mp->GetObservations();
            const auto it = obs.find(kf[s]);
            reg_out[off[s] + j] = it != obs.end() && (int)it->second == j;
        }
    }
    out.insert(out.end(), pool_out.begin(), pool_out.end());
    out.insert(out.end(), reg_out.begin(), reg_out.end());
    out.insert(out.end(), cos_out.begin(), cos_out.end());
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(int32_t), out.size(), f);
    std::fclose(f);
    return 0;
}
