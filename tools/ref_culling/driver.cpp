/*
 * tools/ref_culling/driver.cpp - a world of tests/kf_culling_cases.py through the reference's own LocalMapping::KeyFrameCulling, with its
 * KeyFrame::SetBadFlag and MapPoint::EraseObservation / SetBadFlag: src/LocalMapping.cpp, src/KeyFrame.cpp and src/MapPoint.cpp compiled
 * unmodified against this folder's stand-in headers.  What LocalMapping.cpp names and culling never reaches (Optimizer, ORBmatcher, LoopClosing)
 * is defined here and aborts.  Usage: ref_culling world.bin out.bin (the layouts: kf_culling_cases.world_bytes / run_driver).
 * The keyframes are laid out in one block in (order_key, slot) order, so that std::map<KeyFrame*, ...> and std::set<KeyFrame*> walk them in that
 * order.  The protected members are reached by the define below; the sources themselves are compiled as they are.  AUTHORING TOOLING ONLY.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
static void unreachable(const char *what) { std::fprintf(stderr, "ref_culling: %s was reached\n", what); std::abort(); }
ORBmatcher::ORBmatcher(float, bool) { unreachable("ORBmatcher"); }
int ORBmatcher::DescriptorDistance(const cv::Mat &, const cv::Mat &) { unreachable("DescriptorDistance"); return 0; }
int ORBmatcher::SearchForTriangulation(KeyFrame *, KeyFrame *, cv::Mat, std::vector<std::pair<size_t, size_t>> &, const bool) { unreachable("SearchForTriangulation"); return 0; }
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
    const int S = hd[0], n_rows = hd[1], pool = hd[2], C = hd[3], n_cand = hd[4], monocular = hd[5], first_slot = hd[6], has_ref = hd[7];
    const auto state = take<int32_t>(p, S);
    const auto key = take<int64_t>(p, S);
    const auto off = take<int32_t>(p, S), len = take<int32_t>(p, S), pts = take<int32_t>(p, pool), reg = take<int32_t>(p, pool), parent = take<int32_t>(p, S),
               bad = take<int32_t>(p, n_rows), octave = take<int32_t>(p, pool), stereo = take<int32_t>(p, pool);
    const auto depth = take<float>(p, pool), th_depth = take<float>(p, S);
    const auto not_erase = take<int32_t>(p, S), ref_slot = take<int32_t>(p, n_rows);
    const auto conn_len = take<int32_t>(p, S), conn_slot = take<int32_t>(p, (size_t)S * C), conn_weight = take<int32_t>(p, (size_t)S * C),
               ord_len = take<int32_t>(p, S), ord_slot = take<int32_t>(p, (size_t)S * C), ord_weight = take<int32_t>(p, (size_t)S * C), cand = take<int32_t>(p, n_cand);

    Map map;
    KeyFrameDatabase db;
    // one block, the present slots in (order_key, slot) order, then the current keyframe and a keyframe that stands for "none of the world's"
    std::vector<int> order;
    for (int s = 0; s < S; s++)
        if (state[s] != 0) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
    KeyFrame *block = static_cast<KeyFrame *>(::operator new(sizeof(KeyFrame) * (order.size() + 2)));
    std::vector<KeyFrame *> kf(S, nullptr);
    std::map<KeyFrame *, int> slot_of;
    std::vector<MapPoint *> point(n_rows, nullptr);
    auto run_ok = [&](int s) { return off[s] >= 0 && len[s] >= 0 && off[s] + len[s] <= pool; };
    Frame none_frame;
    KeyFrame *none = new (block + order.size() + 1) KeyFrame(none_frame, &map, &db);
    for (int r = 0; r < n_rows; r++) {
        point[r] = new MapPoint(cv::Mat(), none, &map);
        point[r]->mbBad = bad[r] != 0;
    }
    for (size_t i = 0; i < order.size(); i++) {
        const int s = order[i];
        Frame fr;
        if (run_ok(s)) {
            fr.N = len[s];
            for (int j = 0; j < len[s]; j++) {
                const int e = off[s] + j, r = pts[e];
                cv::KeyPoint kp;
                kp.octave = octave[e];
                fr.mvKeys.push_back(kp); fr.mvKeysUn.push_back(kp);
                fr.mvuRight.push_back(stereo[e] ? 1.0f : -1.0f);
                fr.mvDepth.push_back(depth[e]);
                fr.mvpMapPoints.push_back(r >= 0 && r < n_rows ? point[r] : nullptr);
            }
        }
        fr.mThDepth = th_depth[s];
        kf[s] = new (block + i) KeyFrame(fr, &map, &db);
        kf[s]->mnId = s == first_slot ? 0 : s + 1;
        kf[s]->mbBad = state[s] != 1;
        kf[s]->mbNotErase = not_erase[s] != 0;
        slot_of[kf[s]] = s;
    }
    for (int s = 0; s < S; s++) {
        if (!kf[s]) continue;
        if (state[s] == 1 && run_ok(s))
            for (int j = 0; j < len[s]; j++) {
                const int e = off[s] + j, r = pts[e];
                if (r >= 0 && r < n_rows && !bad[r] && reg[e]) point[r]->AddObservation(kf[s], j);
            }
        kf[s]->mpParent = parent[s] >= 0 && parent[s] < S ? kf[parent[s]] : nullptr;
        if (kf[s]->mpParent) kf[s]->mpParent->mspChildrens.insert(kf[s]);
        for (int j = 0; j < conn_len[s]; j++) kf[s]->mConnectedKeyFrameWeights[kf[conn_slot[(size_t)s * C + j]]] = conn_weight[(size_t)s * C + j];
        for (int j = 0; j < ord_len[s]; j++) {
            kf[s]->mvpOrderedConnectedKeyFrames.push_back(kf[ord_slot[(size_t)s * C + j]]);
            kf[s]->mvOrderedWeights.push_back(ord_weight[(size_t)s * C + j]);
        }
    }
    if (has_ref)
        for (int r = 0; r < n_rows; r++) point[r]->mpRefKF = ref_slot[r] >= 0 && ref_slot[r] < S && kf[ref_slot[r]] ? kf[ref_slot[r]] : none;
    Frame cur_frame;
    KeyFrame *current = new (block + order.size()) KeyFrame(cur_frame, &map, &db);      // its list is the candidates: the copy of :644
    for (int i = 0; i < n_cand; i++) current->mvpOrderedConnectedKeyFrames.push_back(kf[cand[i]]);

    LocalMapping mapper(&map, monocular != 0);
    mapper.mpCurrentKeyFrame = current;
    mapper.KeyFrameCulling();

    std::vector<int32_t> out;
    for (int s = 0; s < S; s++) out.push_back(kf[s] ? (kf[s]->isBad() ? (state[s] == 1 ? 2 : state[s]) : 1) : 0);
    for (int s = 0; s < S; s++) out.push_back(kf[s] && kf[s]->mpParent ? slot_of[kf[s]->mpParent] : parent[s]);
    for (int s = 0; s < S; s++) out.push_back(kf[s] ? (int)kf[s]->mbToBeErased : 0);
    std::vector<int32_t> pool_out(pts), reg_out(reg);
    for (int s = 0; s < S; s++) {
        if (!kf[s] || !run_ok(s)) continue;
        const std::vector<MapPoint *> now = kf[s]->GetMapPointMatches();
        for (int j = 0; j < len[s]; j++) {
            const int e = off[s] + j, r = pts[e];
            if (r < 0 || r >= n_rows) continue;
            if (!now[j]) pool_out[e] = -1;
            const bool was = state[s] == 1 && !bad[r] && reg[e];
            if (was) {
                const std::map<KeyFrame *, size_t> obs = point[r]->GetObservations();
                const auto it = obs.find(kf[s]);
                reg_out[e] = it != obs.end() && (int)it->second == j;
            }
        }
    }
    out.insert(out.end(), pool_out.begin(), pool_out.end());
    out.insert(out.end(), reg_out.begin(), reg_out.end());
    for (int r = 0; r < n_rows; r++) out.push_back(point[r]->isBad());
    for (int r = 0; r < n_rows; r++) out.push_back(point[r]->Observations());
    for (int r = 0; r < n_rows; r++) {           // the same number from the observations themselves
        int n = 0;
        for (auto &o : point[r]->GetObservations()) n += o.first->mvuRight[o.second] >= 0 ? 2 : 1;
        out.push_back(n);
    }
    for (int r = 0; r < n_rows; r++) {
        KeyFrame *k = point[r]->GetReferenceKeyFrame();
        out.push_back(!has_ref ? 0 : k == none ? ref_slot[r] : slot_of.count(k) ? slot_of[k] : -1);       // (begin() of an emptied map: no keyframe)
    }
    std::vector<int32_t> lens[2], slots[2], weights[2];
    for (int s = 0; s < S; s++) {
        std::vector<int32_t> cs(C, 0), cw(C, 0), os(C, 0), ow(C, 0);
        int nc = 0, no = 0;
        if (kf[s]) {
            for (auto &kw : kf[s]->mConnectedKeyFrameWeights) { cs[nc] = slot_of[kw.first]; cw[nc] = kw.second; nc++; }
            const std::vector<KeyFrame *> ord = kf[s]->GetVectorCovisibleKeyFrames();
            for (KeyFrame *o : ord) { os[no] = slot_of[o]; ow[no] = kf[s]->mvOrderedWeights[no]; no++; }
        }
        lens[0].push_back(nc); lens[1].push_back(no);
        slots[0].insert(slots[0].end(), cs.begin(), cs.end()); weights[0].insert(weights[0].end(), cw.begin(), cw.end());
        slots[1].insert(slots[1].end(), os.begin(), os.end()); weights[1].insert(weights[1].end(), ow.begin(), ow.end());
    }
    for (int k = 0; k < 2; k++) {
        out.insert(out.end(), lens[k].begin(), lens[k].end());
        out.insert(out.end(), slots[k].begin(), slots[k].end());
        out.insert(out.end(), weights[k].begin(), weights[k].end());
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(int32_t), out.size(), f);
    std::fclose(f);
    return 0;
}
