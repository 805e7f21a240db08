// update_local_keyframes.cpp - one Tracking::TrackLocalMap step of a monocular frame through the C++ shim, twice, over a small map of its own:
// the host path - Tracking::UpdateLocalKeyFrames as the reference runs it (Tracking.cpp:1844-1952: votes through the points' observations into a
// std::map<KeyFrame*, int>, the first list, the walk over neighbours, children and parents), the keyframes' rows concatenated on the host, then
// Jetson_SLAM::UpdateLocalPoints with that host kf_start - and the device path: Jetson_SLAM::UpdateLocalKeyFrames over a jsorb::KeyframeGraph,
// then UpdateLocalPoints over its list, with no host list in between.  Both end in SearchLocalPoints.  Checks that the list, the reference
// keyframe, the local map and the matches agree.
// Usage: update_local_keyframes            (no input: the image and the map are made here)
// Exit status 0: the two paths agree (and something matched); 1: they differ.
// Build: g++ -std=c++17 -I include examples/update_local_keyframes.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "jsorb_compat.hpp"

#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48

using orb_cuda::SyncedMem;

static unsigned rnd_state = 12345u;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

struct KeyFrame;
struct MapPoint {
    int row = 0;
    bool bad = false;
    std::map<KeyFrame *, size_t> mObservations;
};
struct KeyFrame {
    int slot = 0;
    bool bad = false;
    long mnTrackReferenceForFrame = 0;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> mspChildrens;
    KeyFrame *mpParent = nullptr;
};

int main()
{
    const int H = 240, W = 320, L = 3, tile = 15, n_kf = 24;
    std::vector<unsigned char> image((size_t)H * W);
    for (auto &p : image) p = 90 + rnd() % 12;
    for (int b = 0; b < 260; b++) {                      // rectangles of random grey: corners for FAST
        const int x0 = rnd() % (W - 8), y0 = rnd() % (H - 8), w = 4 + rnd() % 30, h = 4 + rnd() % 30, g = rnd() % 256;
        for (int y = y0; y < y0 + h && y < H; y++)
            for (int x = x0; x < x0 + w && x < W; x++) image[(size_t)y * W + x] = (unsigned char)g;
    }
    try {
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, L, 9, 14, 7, 20, std::string(), tile, tile, false, false, false, true);
        SyncedMem<int> kp_gpu;
        SyncedMem<unsigned char> desc_gpu;
        ex.extract(image.data(), W, kp_gpu, desc_gpu);
        std::vector<jsorb_keypoint> keys;
        std::vector<unsigned char> desc;
        Jetson_SLAM::UnpackFrame(ex, keys, desc);
        const int N = (int)keys.size();
        if (N < 100) { fprintf(stderr, "only %d keypoints\n", N); return 1; }

        // ---- the map: one point per keypoint at depth 4 in front of the identity pose; keyframes that see runs of them ----
        const int n_rows = N;
        const float fx = 300.0f, fy = 300.0f, cx = W / 2.0f, cy = H / 2.0f, logsf = logf(1.2f);
        std::vector<jsorb_map_point_record> rec(n_rows);
        std::vector<int32_t> all_rows(n_rows);
        std::vector<MapPoint> mps(n_rows);
        for (int r = 0; r < n_rows; r++) {
            const float z = 4.0f, X = (keys[r].x - cx) * z / fx, Y = (keys[r].y - cy) * z / fy, d = sqrtf(X * X + Y * Y + z * z);
            const float maxd = d * jsorb_scale(ex.handle(), keys[r].octave) * 0.999f;
            rec[r] = jsorb_map_point_record{{X, Y, z}, {X / d, Y / d, z / d}, maxd, maxd * 1.2f, maxd / jsorb_scale(ex.handle(), L - 1) * 0.8f, (uint8_t)(r % 29 == 0), {0, 0, 0}};
            all_rows[r] = r;
            mps[r].row = r;
            mps[r].bad = rec[r].bad != 0;
        }
        std::vector<KeyFrame> kfs(n_kf);                 // (their addresses ascend with the slot: std::map's order is the slot order here)
        for (int k = 0; k < n_kf; k++) {
            KeyFrame &kf = kfs[k];
            kf.slot = k;
            kf.bad = k == 5;
            const int first = (k * n_rows) / (n_kf + 6), len = n_rows / 4;
            for (int j = 0; j < len; j++) {
                MapPoint *p = rnd() % 5 == 0 ? nullptr : &mps[(first + j) % n_rows];
                kf.mvpMapPoints.push_back(p);
                if (p && !(k == 9 && j % 2)) p->mObservations[&kf] = j;      // keyframe 9: a new keyframe, half of whose points LocalMapping has not registered yet
            }
            for (int j = 1; j <= 3; j++) kf.mvpOrderedConnectedKeyFrames.push_back(&kfs[(k + 7 * j) % n_kf]);
            if (k > 0) { kf.mpParent = &kfs[(k - 1) / 2]; kfs[(k - 1) / 2].mspChildrens.insert(&kf); }
        }
        std::vector<MapPoint *> frame_points(N, nullptr);    // mCurrentFrame.mvpMapPoints: what the motion model tracked - points of keyframes 8 .. 13
        for (int k = 0; k < N; k++)
            if (rnd() % 3 == 0) frame_points[k] = &mps[((8 + rnd() % 6) * n_rows) / (n_kf + 6) + rnd() % (n_rows / 4)];

        // ---- the host path: Tracking.cpp:1844-1952 ----
        const long frame_id = 7;
        std::vector<KeyFrame *> mvpLocalKeyFrames;
        KeyFrame *mpReferenceKF = nullptr;
        {
            std::map<KeyFrame *, int> keyframeCounter;
            for (int i = 0; i < N; i++)
                if (frame_points[i]) {
                    MapPoint *pMP = frame_points[i];
                    if (!pMP->bad) {
                        for (auto &o : pMP->mObservations) keyframeCounter[o.first]++;
                    } else
                        frame_points[i] = nullptr;
                }
            int max = 0;
            KeyFrame *pKFmax = nullptr;
            for (auto &it : keyframeCounter) {
                KeyFrame *pKF = it.first;
                if (pKF->bad) continue;
                if (it.second > max) { max = it.second; pKFmax = pKF; }
                mvpLocalKeyFrames.push_back(pKF);
                pKF->mnTrackReferenceForFrame = frame_id;
            }
            const size_t end = mvpLocalKeyFrames.size();
            for (size_t i = 0; i < end; i++) {
                if (mvpLocalKeyFrames.size() > 80) break;
                KeyFrame *pKF = mvpLocalKeyFrames[i];
                for (KeyFrame *n : pKF->mvpOrderedConnectedKeyFrames)
                    if (!n->bad && n->mnTrackReferenceForFrame != frame_id) { mvpLocalKeyFrames.push_back(n); n->mnTrackReferenceForFrame = frame_id; break; }
                for (KeyFrame *c : pKF->mspChildrens)
                    if (!c->bad && c->mnTrackReferenceForFrame != frame_id) { mvpLocalKeyFrames.push_back(c); c->mnTrackReferenceForFrame = frame_id; break; }
                KeyFrame *p = pKF->mpParent;
                if (p && p->mnTrackReferenceForFrame != frame_id) { mvpLocalKeyFrames.push_back(p); p->mnTrackReferenceForFrame = frame_id; break; }
            }
            if (pKFmax) mpReferenceKF = pKFmax;
        }
        std::vector<int32_t> kf_start(1, 0), kf_point_row, frame_row(N, -1);      // the host concatenation the local map took until now
        for (KeyFrame *kf : mvpLocalKeyFrames) {
            for (MapPoint *p : kf->mvpMapPoints) kf_point_row.push_back(p ? p->row : -1);
            kf_start.push_back((int32_t)kf_point_row.size());
        }
        for (int k = 0; k < N; k++)
            if (frame_points[k]) frame_row[k] = frame_points[k]->row;

        // ---- the device side of the map: the table and the graph, written where the reference changes the map ----
        jsorb::MapPointTable table(n_rows);
        table.scatter(all_rows, rec, jsorb_get_stream(ex.handle()));
        table.set_descriptors(0, n_rows, desc.data());
        jsorb::KeyframeGraph graph(32, n_kf * (n_rows / 4), 64);
        for (KeyFrame &kf : kfs) {
            std::vector<int32_t> rows, nb, ch;
            std::vector<unsigned char> reg;
            for (MapPoint *p : kf.mvpMapPoints) {
                rows.push_back(p ? p->row : -1);
                reg.push_back(p && p->mObservations.count(&kf) ? 1 : 0);
            }
            graph.set_keyframe(kf.slot, rows, (int64_t)(intptr_t)&kf, kf.bad ? jsorb::KeyframeGraph::BAD : jsorb::KeyframeGraph::GOOD, &reg);
            for (KeyFrame *n : kf.mvpOrderedConnectedKeyFrames) nb.push_back(n->slot);
            for (KeyFrame *c : kf.mspChildrens) ch.push_back(c->slot);
            graph.set_neighbours(kf.slot, nb);
            graph.set_children(kf.slot, ch);
            graph.set_parent(kf.slot, kf.mpParent ? kf.mpParent->slot : -1);
        }
        // the frame's rows as the host found them (bad points included: both calls drop them themselves)
        SyncedMem<int> frame_rows_gpu, kf_rows_gpu;
        frame_rows_gpu.resize(N);
        for (int k = 0; k < N; k++) frame_rows_gpu.cpu_data()[k] = frame_row[k];
        frame_rows_gpu.to_gpu();
        kf_rows_gpu.resize((int)kf_point_row.size() > 0 ? (int)kf_point_row.size() : 1);
        memcpy(kf_rows_gpu.cpu_data(), kf_point_row.data(), 4 * kf_point_row.size());
        kf_rows_gpu.to_gpu();

        jsorb_frustum_params fp{};
        fp.Rcw[0] = fp.Rcw[4] = fp.Rcw[8] = 1.0f;
        fp.fx = fx; fp.fy = fy; fp.cx = cx; fp.cy = cy;
        fp.minX = 0; fp.maxX = W; fp.minY = 0; fp.maxY = H; fp.nScaleLevels = L;
        fp.logScaleFactor = logsf; fp.viewCosAngle = 0.5f;
        jsorb_search_params prm{1.0f, 0.8f, 100, 0.0f, 0.0f, 0.0f, (float)FRAME_GRID_COLS / W, (float)FRAME_GRID_ROWS / H, FRAME_GRID_COLS, FRAME_GRID_ROWS};
        const int capacity = (int)kf_point_row.size() + 16;

        // host list + host concatenation -> the local map -> the matcher
        jsorb::LocalMapPoints pts_host;
        std::vector<int> match_host;
        const int n_host = Jetson_SLAM::UpdateLocalPoints(ex, table, fp, kf_start, kf_rows_gpu.gpu_data(), frame_rows_gpu.gpu_data(), capacity, pts_host);
        const int m_host = Jetson_SLAM::SearchLocalPoints(ex, prm, pts_host, nullptr, match_host);

        // the two device calls -> the matcher
        jsorb::LocalKeyFrames local(84, (int)kf_point_row.size() + 16);
        jsorb::LocalMapPoints pts_dev;
        std::vector<int> match_dev;
        const int n_local = Jetson_SLAM::UpdateLocalKeyFrames(ex, graph, table, frame_rows_gpu.gpu_data(), N, local);
        const int n_dev = Jetson_SLAM::UpdateLocalPoints(ex, table, fp, local, frame_rows_gpu.gpu_data(), capacity, pts_dev);
        const int m_dev = Jetson_SLAM::SearchLocalPoints(ex, prm, pts_dev, nullptr, match_dev);

        bool same = n_local == (int)mvpLocalKeyFrames.size() && mpReferenceKF && local.ref_slot == mpReferenceKF->slot &&
                    local.counts[4] == (int)kf_point_row.size() && !local.counts[5] && !local.counts[6] && !local.counts[7];
        for (int i = 0; same && i < n_local; i++) same = local.slots[i] == mvpLocalKeyFrames[i]->slot;
        same = same && n_host == n_dev && m_host == m_dev && pts_host.point_row == pts_dev.point_row && match_host == match_dev &&
               !memcmp(pts_host.counts, pts_dev.counts, 4 * sizeof(int32_t));
        printf("%s keypoints=%d local_keyframes=%d/%d ref=%d/%d entries=%d nToMatch=%d/%d nmatches=%d/%d\n", same ? "ok" : "MISMATCH", N,
               (int)mvpLocalKeyFrames.size(), n_local, mpReferenceKF ? mpReferenceKF->slot : -1, local.ref_slot, (int)kf_point_row.size(), n_host, n_dev, m_host, m_dev);
        return same && m_dev > 0 && n_local > 6 ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
