// update_map_points.cpp - one fusing step of LocalMapping::SearchInNeighbors (LocalMapping.cpp:497-504: the current keyframe's map points into its
// target keyframes) with the map points' descriptor table ON THE DEVICE.  The first image plays the current keyframe, the other three its targets.
// One Jetson_SLAM::Fuse call searches every point in every target; the loop that follows replays the head test (ORBmatcher.cpp:833-837) and the tail
// (:938-958) keyframe by keyframe over a small map of the example's own.  MapPoint::Replace ends with ComputeDistinctiveDescriptors() on the
// survivor (MapPoint.cpp:243), and that is what this example is about: after the replay of a keyframe the survivors are refreshed by ONE
// Jetson_SLAM::ComputeDistinctiveDescriptors call - their observations as a CSR, out_row = their rows of the table, `changed` from the device - and
// the changed points of the list are fused into the keyframes still to come straight from the table, no descriptor crossing the bus.
// The example checks itself: a twin of the map runs the same step with the host loop examples/search_in_neighbors.cpp has (the sort-based
// MapPoint::ComputeDistinctiveDescriptors, inside Replace, timed) and descriptors uploaded from the host for every renewed search; the two maps must
// end up the same - every slot, every point's state, every good point's 32 descriptor bytes against the table as downloaded - and every
// renewed search must have returned the same matches.
// Usage: update_map_points H W L tile th_fast current.raw t0.raw t1.raw t2.raw        (*.raw: H*W bytes each)
// Build: g++ -std=c++17 -I include examples/update_map_points.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "jsorb_compat.hpp"

using orb_cuda::SyncedMem;

template <class T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

// ---- the example's map (the bookkeeping of examples/search_in_neighbors.cpp) ----
struct KeyFrame;
struct ById { bool operator()(const KeyFrame *a, const KeyFrame *b) const; };
struct MapPoint {
    int id = 0;
    float P[3], N[3], max_distance, min_dist_inv, max_dist_inv;
    unsigned char desc[32];                      // the twin's mDescriptor; the device run keeps the table's row `id` instead
    bool bad = false;
    int nObs = 0;
    std::map<KeyFrame *, int, ById> obs;         // walked in the order of the keyframes' ids (the reference: in pointer order)
    bool IsInKeyFrame(KeyFrame *kf) const { return obs.count(kf) != 0; }
    void AddObservation(KeyFrame *kf, int idx);
};
struct KeyFrame {
    int id = 0;
    std::vector<float> x, y, uright;
    std::vector<int> octave;
    std::vector<unsigned char> desc;
    std::vector<MapPoint *> mps;
    float T[15];                                 // Rcw row-major, tcw, Ow
    int n() const { return (int)x.size(); }
};
inline bool ById::operator()(const KeyFrame *a, const KeyFrame *b) const { return a->id < b->id; }
void MapPoint::AddObservation(KeyFrame *kf, int idx)      // MapPoint.cpp:129-140
{
    if (obs.count(kf)) return;
    obs[kf] = idx;
    nObs += kf->uright[idx] >= 0 ? 2 : 1;
}

static int hamming(const unsigned char *a, const unsigned char *b)
{
    int d = 0;
    for (int w = 0; w < 4; w++) {
        unsigned long long p, q;
        memcpy(&p, a + 8 * w, 8);
        memcpy(&q, b + 8 * w, 8);
        d += __builtin_popcountll(p ^ q);
    }
    return d;
}

// MapPoint.cpp:273-338 on the host, the loop of examples/search_in_neighbors.cpp: a sort per observation
static void host_distinctive(MapPoint &mp)
{
    if (mp.bad || mp.obs.empty()) return;
    std::vector<const unsigned char *> d;
    for (auto &o : mp.obs) d.push_back(&o.first->desc[32 * (size_t)o.second]);
    const size_t N = d.size();
    int bestMedian = INT_MAX;
    size_t best = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> row(N);
        for (size_t j = 0; j < N; j++) row[j] = hamming(d[i], d[j]);
        std::sort(row.begin(), row.end());
        const int median = row[(size_t)(0.5 * (double)(N - 1))];
        if (median < bestMedian) { bestMedian = median; best = i; }
    }
    memcpy(mp.desc, d[best], 32);
}

// one run of the step: the map, and how it refreshes a survivor - at once on the host (the twin), or collected for the device call
struct Run {
    bool on_device;
    std::vector<MapPoint *> survivors;           // of the keyframe being replayed, in the order Replace named them
    double host_loop_us = 0;
    void Replace(MapPoint *gone, MapPoint *pMP)  // MapPoint.cpp:208-246
    {
        if (pMP->id == gone->id) return;
        gone->bad = true;
        std::map<KeyFrame *, int, ById> mine;
        mine.swap(gone->obs);
        for (auto &o : mine) {
            if (!pMP->IsInKeyFrame(o.first)) {
                o.first->mps[o.second] = pMP;
                pMP->AddObservation(o.first, o.second);
            } else {
                o.first->mps[o.second] = nullptr;
            }
        }
        if (on_device) { survivors.push_back(pMP); return; }      // :243, deferred to one call behind the keyframe
        const auto t0 = std::chrono::steady_clock::now();
        host_distinctive(*pMP);
        host_loop_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    void fuse_tail(KeyFrame *pKF, MapPoint *pMP, int bestIdx)     // ORBmatcher.cpp:938-958
    {
        MapPoint *pMPinKF = pKF->mps[bestIdx];
        if (pMPinKF) {
            if (!pMPinKF->bad) {
                if (pMPinKF->nObs > pMP->nObs) Replace(pMP, pMPinKF);
                else Replace(pMPinKF, pMP);
            }
        } else {
            pMP->AddObservation(pKF, bestIdx);
            pKF->mps[bestIdx] = pMP;
        }
    }
};

template <class T, class U> static void upload(SyncedMem<T> &m, const std::vector<U> &v)
{
    m.resize(v.empty() ? 1 : (int)v.size());
    for (size_t i = 0; i < v.size(); i++) m.cpu_data()[i] = (T)v[i];
    m.to_gpu();
}

// the float arrays of some map points as the device arrays of jsorb::FusePoints; the descriptors are the caller's
struct DevicePoints {
    SyncedMem<float> a[9];
    jsorb::FusePoints side;
    void set(const std::vector<MapPoint *> &pts, const unsigned char *desc_gpu)
    {
        std::vector<float> host[9];
        for (const MapPoint *m : pts) {
            const float f[9] = {m->P[0], m->P[1], m->P[2], m->N[0], m->N[1], m->N[2], m->max_distance, m->min_dist_inv, m->max_dist_inv};
            for (int k = 0; k < 9; k++) host[k].push_back(f[k]);
        }
        for (int k = 0; k < 9; k++) upload(a[k], host[k]);
        side.n = (int)pts.size();
        side.Px = a[0].gpu_data(); side.Py = a[1].gpu_data(); side.Pz = a[2].gpu_data(); side.Nx = a[3].gpu_data(); side.Ny = a[4].gpu_data();
        side.Nz = a[5].gpu_data(); side.max_distance = a[6].gpu_data(); side.min_dist_inv = a[7].gpu_data(); side.max_dist_inv = a[8].gpu_data();
        side.descriptors = desc_gpu;
    }
};

// keyframes one after the other as the device arrays of jsorb::FuseKeyframes
struct DeviceKeyframes {
    SyncedMem<float> x, y, uright;
    SyncedMem<int> octave;
    SyncedMem<unsigned char> desc;
    jsorb::FuseKeyframes side;
    std::vector<int32_t> kf_start;
    std::vector<float> Rcw, tcw, Ow;
    void set(const std::vector<KeyFrame *> &kfs)
    {
        std::vector<float> vx, vy, vr;
        std::vector<int> vo;
        std::vector<unsigned char> vd;
        kf_start.assign(1, 0);
        for (const KeyFrame *k : kfs) {
            vx.insert(vx.end(), k->x.begin(), k->x.end()); vy.insert(vy.end(), k->y.begin(), k->y.end());
            vr.insert(vr.end(), k->uright.begin(), k->uright.end()); vo.insert(vo.end(), k->octave.begin(), k->octave.end());
            vd.insert(vd.end(), k->desc.begin(), k->desc.end());
            kf_start.push_back((int32_t)vx.size());
            Rcw.insert(Rcw.end(), k->T, k->T + 9); tcw.insert(tcw.end(), k->T + 9, k->T + 12); Ow.insert(Ow.end(), k->T + 12, k->T + 15);
        }
        upload(x, vx); upload(y, vy); upload(uright, vr); upload(octave, vo); upload(desc, vd);
        side.x = x.gpu_data(); side.y = y.gpu_data(); side.uright = uright.gpu_data(); side.octave = octave.gpu_data(); side.descriptors = desc.gpu_data();
    }
    jsorb::FusePoses poses(int k0) const { jsorb::FusePoses p; p.Rcw = Rcw.data() + 9 * k0; p.tcw = tcw.data() + 3 * k0; p.Ow = Ow.data() + 3 * k0; return p; }
};

struct Step {
    int fused = 0, refreshed = 0, changed = 0, researched = 0;
    std::vector<int32_t> renewed;                // every renewed search's best_idx and best_dist, in order
};

// the step on one map.  all: every keyframe (id order) on the device - its descriptors are what obs_row points into; targets: all but the first.
// table: the device table of every map point's descriptor, row = id (the device run reads and refreshes it; the twin only uploads into a copy).
static Step run_step(jsorb::KeyframeMatcher &matcher, const jsorb_fuse_params &prm, Run &run, const std::vector<MapPoint *> &pts,
                     const std::vector<KeyFrame *> &kfs, const DeviceKeyframes &all, SyncedMem<unsigned char> &table, int n_map)
{
    Step st;
    const int n = (int)pts.size(), n_kf = (int)kfs.size() - 1;
    DevicePoints dp;
    // the list is the current keyframe's points, whose ids are 0 .. n - 1: the head of the table IS the list's descriptor array
    for (int i = 0; i < n; i++) if (pts[i]->id != i) throw std::runtime_error("the list is not the head of the table");
    dp.set(pts, table.gpu_data());
    std::vector<unsigned char> skip((size_t)n_kf * n, 0);      // nothing of the current keyframe is in a target yet
    SyncedMem<unsigned char> skip_gpu;
    upload(skip_gpu, skip);
    jsorb::FuseKeyframes tk = all.side;                         // the targets: the keyframes behind the first
    const int t0 = all.kf_start[1];
    tk.x += t0; tk.y += t0; tk.uright += t0; tk.octave += t0; tk.descriptors += 32 * (size_t)t0;
    std::vector<int32_t> rel;
    for (int k = 1; k <= n_kf + 1; k++) rel.push_back(all.kf_start[k] - t0);
    std::vector<int32_t> best_idx, best_dist;
    Jetson_SLAM::Fuse(matcher, prm, dp.side, n_kf, rel.data(), tk, all.poses(1), skip_gpu.gpu_data(), best_idx, best_dist);
    std::vector<unsigned char> searched_with((size_t)32 * n);   // the twin's "last searched with"
    for (int i = 0; i < n; i++) memcpy(&searched_with[32 * (size_t)i], pts[i]->desc, 32);
    for (int k = 0; k < n_kf; k++) {
        KeyFrame *pKF = kfs[k + 1];
        run.survivors.clear();
        for (int i = 0; i < n; i++) {
            MapPoint *pMP = pts[i];
            if (pMP->bad || pMP->IsInKeyFrame(pKF)) continue;          // :833-837 on the live map
            const int bestIdx = best_idx[(size_t)k * n + i];
            if (bestIdx < 0) continue;                                   // :939
            run.fuse_tail(pKF, pMP, bestIdx);
            st.fused++;
        }
        std::vector<MapPoint *> again;                                   // the points of the list to search in the keyframes still to come
        if (run.on_device) {
            // the survivors that are still good, once each: their observations in map order (no keyframe here is bad) as a CSR into `all`
            std::vector<MapPoint *> S;
            std::set<int> seen;
            for (MapPoint *p : run.survivors) if (!p->bad && seen.insert(p->id).second) S.push_back(p);
            if (!S.empty()) {
                std::vector<int32_t> obs_start(1, 0), obs_row, out_row;
                for (MapPoint *p : S) {
                    for (auto &o : p->obs) obs_row.push_back(all.kf_start[o.first->id] + o.second);
                    obs_start.push_back((int32_t)obs_row.size());
                    out_row.push_back(p->id);
                }
                SyncedMem<int32_t> d_start, d_row, d_out;
                SyncedMem<unsigned char> d_changed;
                upload(d_start, obs_start); upload(d_row, obs_row); upload(d_out, out_row);
                d_changed.resize((int)S.size());
                jsorb::Observations obs;
                obs.n = (int)S.size(); obs.n_obs = (int)obs_row.size(); obs.n_rows = all.kf_start.back();
                obs.obs_start = d_start.gpu_data(); obs.obs_row = d_row.gpu_data(); obs.kf_descriptors = all.side.descriptors; obs.out_row = d_out.gpu_data();
                std::vector<int32_t> bo, bm;
                if (Jetson_SLAM::ComputeDistinctiveDescriptors(matcher, obs, table.gpu_data(), n_map, d_changed.gpu_data(), bo, bm) != (int)S.size())
                    throw std::runtime_error("a survivor without a winner");
                d_changed.to_cpu();
                st.refreshed += (int)S.size();
                for (size_t s = 0; s < S.size(); s++) {
                    if (!d_changed.cpu_data()[s]) continue;
                    st.changed++;
                    if (S[s]->id < n) again.push_back(S[s]);
                }
                std::sort(again.begin(), again.end(), [](const MapPoint *a, const MapPoint *b) { return a->id < b->id; });
            }
        } else {
            for (int i = 0; i < n; i++)
                if (!pts[i]->bad && memcmp(pts[i]->desc, &searched_with[32 * (size_t)i], 32) != 0) again.push_back(pts[i]);
        }
        if (again.empty() || k + 1 == n_kf) continue;
        // the renewed search: those points against the keyframes k + 1 .., the head test as the skip mask
        const int m = (int)again.size(), rest = n_kf - (k + 1);
        SyncedMem<unsigned char> sub_desc;
        sub_desc.resize(32 * m);
        for (int j = 0; j < m; j++) {
            if (run.on_device) {
                if (jsorb_mem_d2d(sub_desc.gpu_data() + 32 * (size_t)j, table.gpu_data() + 32 * (size_t)again[j]->id, 32) != JSORB_OK) throw std::runtime_error("jsorb_mem_d2d");
            } else {
                memcpy(sub_desc.cpu_data() + 32 * (size_t)j, again[j]->desc, 32);
            }
        }
        if (!run.on_device) sub_desc.to_gpu();
        DevicePoints sub;
        sub.set(again, sub_desc.gpu_data());
        std::vector<unsigned char> sk((size_t)rest * m);
        for (int a = 0; a < rest; a++)
            for (int j = 0; j < m; j++) sk[(size_t)a * m + j] = again[j]->bad || again[j]->IsInKeyFrame(kfs[k + 2 + a]);
        SyncedMem<unsigned char> sk_gpu;
        upload(sk_gpu, sk);
        jsorb::FuseKeyframes rk = all.side;
        const int r0 = all.kf_start[k + 2];
        rk.x += r0; rk.y += r0; rk.uright += r0; rk.octave += r0; rk.descriptors += 32 * (size_t)r0;
        std::vector<int32_t> rrel, bi, bd;
        for (int a = k + 2; a <= n_kf + 1; a++) rrel.push_back(all.kf_start[a] - r0);
        Jetson_SLAM::Fuse(matcher, prm, sub.side, rest, rrel.data(), rk, all.poses(k + 2), sk_gpu.gpu_data(), bi, bd);
        for (int a = 0; a < rest; a++)
            for (int j = 0; j < m; j++) {
                best_idx[(size_t)(k + 1 + a) * n + again[j]->id] = bi[(size_t)a * m + j];
                best_dist[(size_t)(k + 1 + a) * n + again[j]->id] = bd[(size_t)a * m + j];
            }
        st.renewed.insert(st.renewed.end(), bi.begin(), bi.end());
        st.renewed.insert(st.renewed.end(), bd.begin(), bd.end());
        st.researched += m;
        for (MapPoint *p : again) memcpy(&searched_with[32 * (size_t)p->id], p->desc, 32);
    }
    return st;
}

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s H W L tile th_fast current.raw t0.raw t1.raw t2.raw\n", argv[0]); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th_fast = atoi(argv[5]);
    std::vector<std::vector<unsigned char>> images(4, std::vector<unsigned char>((size_t)H * W));
    for (int i = 0; i < 4; i++) {
        FILE *f = fopen(argv[6 + i], "rb");
        if (!f || !rd(f, images[i])) { fprintf(stderr, "cannot read %s\n", argv[6 + i]); return 2; }
        fclose(f);
    }
    try {
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, L, 9, 14, 7, th_fast, std::string(), tile, tile, false, false, false, true);
        jsorb_fuse_params prm{};
        prm.th = 3.0f; prm.th_low = 50; prm.check_reprojection = 1;
        prm.fx = prm.fy = (float)W; prm.cx = 0.5f * W; prm.cy = 0.5f * H; prm.bf = 0.1f * W;
        prm.min_x = 0; prm.max_x = (float)W; prm.min_y = 0; prm.max_y = (float)H;
        prm.cols = 64; prm.rows = 48; prm.inv_w = 64.0f / (float)W; prm.inv_h = 48.0f / (float)H;
        prm.log_scale_factor = logf(1.2f); prm.n_levels = L;
        float scale = 1.0f;
        for (int l = 0; l < L; l++) { prm.scale_factor[l] = scale; prm.inv_level_sigma2[l] = 1.0f / (scale * scale); scale *= 1.2f; }
        // the four keyframes and their points, as examples/search_in_neighbors.cpp makes them
        const float shift[4][3] = {{0, 0, 0}, {-0.1f, 0, 0}, {0.002f, -0.001f, 0}, {0.01f, 0, 0.005f}};
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        std::vector<std::unique_ptr<MapPoint>> map;
        for (int k = 0; k < 4; k++) {
            SyncedMem<int> keys;
            SyncedMem<unsigned char> desc;
            ex.extract(images[k].data(), W, keys, desc);
            const int n = jsorb_n_keypoints(ex.handle(), 0);
            kfs.emplace_back(new KeyFrame);
            KeyFrame &kf = *kfs.back();
            kf.id = k;
            const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(kf.T, I, sizeof(I));
            for (int c = 0; c < 3; c++) { kf.T[9 + c] = shift[k][c]; kf.T[12 + c] = -shift[k][c]; }
            const int *soa = keys.cpu_data();
            kf.mps.assign(n, nullptr);
            kf.desc.assign(desc.cpu_data(), desc.cpu_data() + 32 * (size_t)n);
            for (int i = 0; i < n; i++) {
                const float x = (float)soa[i], y = (float)soa[(size_t)n + i], z = 2.0f + 0.5f * (float)(i % 7);
                kf.x.push_back(x);
                kf.y.push_back(y);
                kf.octave.push_back(soa[4 * (size_t)n + i]);
                kf.uright.push_back(i % 2 ? x - prm.bf / z : -1.0f);
                if (i % 3 == 2) continue;
                map.emplace_back(new MapPoint);
                MapPoint &mp = *map.back();
                mp.id = (int)map.size() - 1;
                const float Pc[3] = {(x - prm.cx) * z / prm.fx, (y - prm.cy) * z / prm.fy, z};
                float d2 = 0;
                for (int c = 0; c < 3; c++) { mp.P[c] = Pc[c] - kf.T[9 + c]; d2 += Pc[c] * Pc[c]; }
                const float dist = sqrtf(d2);
                for (int c = 0; c < 3; c++) mp.N[c] = Pc[c] / dist;
                mp.max_distance = dist * prm.scale_factor[kf.octave[i]];
                mp.max_dist_inv = 1.2f * mp.max_distance;
                mp.min_dist_inv = 0.8f * (mp.max_distance / prm.scale_factor[L - 1]);
                memcpy(mp.desc, &kf.desc[32 * (size_t)i], 32);
                mp.AddObservation(&kf, i);
                kf.mps[i] = &mp;
            }
        }
        // the twin map for the host loop: the same keyframes and points, its own pointers
        std::vector<std::unique_ptr<KeyFrame>> kfs2;
        std::vector<std::unique_ptr<MapPoint>> map2;
        for (auto &p : map) map2.emplace_back(new MapPoint(*p));
        for (auto &k : kfs) {
            kfs2.emplace_back(new KeyFrame(*k));
            for (MapPoint *&p : kfs2.back()->mps) if (p) p = map2[p->id].get();
        }
        for (auto &p : map2) {
            std::map<KeyFrame *, int, ById> obs;
            for (auto &o : p->obs) obs[kfs2[o.first->id].get()] = o.second;
            p->obs.swap(obs);
        }
        const int n_map = (int)map.size();
        std::vector<KeyFrame *> K1, K2;
        for (int k = 0; k < 4; k++) { K1.push_back(kfs[k].get()); K2.push_back(kfs2[k].get()); }
        DeviceKeyframes all;
        all.set(K1);
        // the descriptor table: every map point's 32 bytes, row = id, uploaded once
        std::vector<unsigned char> table_host;
        for (auto &p : map) table_host.insert(table_host.end(), p->desc, p->desc + 32);
        SyncedMem<unsigned char> table, table2;
        upload(table, table_host);
        upload(table2, table_host);
        std::vector<MapPoint *> list, list2;                        // vpMapPointMatches without its NULL slots
        for (MapPoint *p : kfs[0]->mps) if (p) list.push_back(p);
        for (MapPoint *p : list) list2.push_back(map2[p->id].get());
        jsorb::KeyframeMatcher matcher;
        Run dev{true}, host{false};
        const Step a = run_step(matcher, prm, dev, list, K1, all, table, n_map);
        const Step b = run_step(matcher, prm, host, list2, K2, all, table2, n_map);
        // the self-check: the maps, the renewed searches, and every good point's descriptor against the table as downloaded
        table.to_cpu();
        bool same = a.fused == b.fused && a.researched == b.researched && a.renewed == b.renewed;
        for (int k = 0; k < 4 && same; k++)
            for (size_t i = 0; i < kfs[k]->mps.size(); i++) {
                const MapPoint *p = kfs[k]->mps[i], *q = kfs2[k]->mps[i];
                if ((p == nullptr) != (q == nullptr) || (p && p->id != q->id)) same = false;
            }
        int good = 0;
        for (int p = 0; p < n_map && same; p++) {
            if (map[p]->bad != map2[p]->bad || map[p]->nObs != map2[p]->nObs) same = false;
            else if (!map[p]->bad) { good++; same = memcmp(table.cpu_data() + 32 * (size_t)p, map2[p]->desc, 32) == 0; }
        }
        printf("keyframes=%d,%d,%d,%d points=%d map=%d good=%d fused=%d refreshed=%d changed=%d researched=%d host_loop_us=%.1f\n", kfs[0]->n(), kfs[1]->n(),
               kfs[2]->n(), kfs[3]->n(), (int)list.size(), n_map, good, a.fused, a.refreshed, a.changed, a.researched, host.host_loop_us);
        if (!same || a.fused < 15 || a.refreshed < 15 || a.changed < 1) { fprintf(stderr, "the device step and the host loop disagree (or nothing was refreshed)\n"); return 1; }
        printf("self-check ok\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
