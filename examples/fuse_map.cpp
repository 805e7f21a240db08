// fuse_map.cpp - both directions of LocalMapping::SearchInNeighbors on the device state through the C++ shim (Jetson_SLAM::FuseMap), then
// UpdateConnections on the same matcher, against the sequential host loop on a twin map: jsorb_fuse for one keyframe at a time, the head test, the
// tail of ORBmatcher::Fuse, MapPoint::Replace / AddObservation and ComputeDistinctiveDescriptors on host vectors, as a binding without the device
// map does it.  The map is made here: a current keyframe with eleven points, three neighbours that see some of them at the same pixels - empty
// slots, slots holding other points with fewer, as many and more observations, a bad point - and one more observer.
// Usage: fuse_map            (no input)
// Exit status 0: the device map, the logs and the covisibility weights equal the twin's; 1: any difference.
// Build: g++ -std=c++17 -I include examples/fuse_map.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

#include "jsorb_compat.hpp"

namespace {

const int S = 6, N_ROWS = 32, CUR = 0, KP = 12;          // slots 1-3: the neighbours, 4: another observer, 5: absent

struct Twin {                                            // the host map: per slot the keyframe's points and registered bytes, per row bad and descriptor
    std::vector<std::vector<int32_t>> mps;
    std::vector<std::vector<unsigned char>> reg, kdesc;  // kdesc: 32 bytes per keypoint
    std::vector<unsigned char> bad, desc;
    std::vector<std::array<int32_t, 4>> events;
    std::vector<std::pair<int, int>> observations(int r) const
    {
        std::vector<std::pair<int, int>> o;
        for (int s = 0; s < (int)mps.size(); s++)
            for (int i = 0; i < (int)mps[s].size(); i++)
                if (mps[s][i] == r && reg[s][i]) o.push_back({s, i});
        return o;
    }
    void descriptor(int q)                               // MapPoint.cpp:273-338, the observers in slot order (order_key ascends with the slot here)
    {
        const auto o = observations(q);
        if (bad[q] || o.empty()) return;
        int best = 0, best_median = 1 << 30;
        for (size_t i = 0; i < o.size(); i++) {
            std::vector<int> d;
            for (size_t j = 0; j < o.size(); j++) {
                int h = 0;
                for (int b = 0; b < 32; b++) h += __builtin_popcount(kdesc[o[i].first][32 * o[i].second + b] ^ kdesc[o[j].first][32 * o[j].second + b]);
                d.push_back(h);
            }
            std::sort(d.begin(), d.end());
            if (d[(o.size() - 1) / 2] < best_median) { best_median = d[(o.size() - 1) / 2]; best = (int)i; }
        }
        std::copy_n(&kdesc[o[best].first][32 * o[best].second], 32, &desc[32 * q]);
    }
    void replace(int p, int q)                           // p->Replace(q), MapPoint.cpp:208-246
    {
        if (p == q) return;
        events.push_back({2, p, q, -1});
        std::map<int, int> in_q;
        for (auto &o : observations(q)) in_q[o.first] = 1;
        for (auto &o : observations(p)) {
            if (in_q.count(o.first)) { mps[o.first][o.second] = -1; reg[o.first][o.second] = 0; }
            else mps[o.first][o.second] = q;
        }
        bad[p] = 1;
        descriptor(q);
    }
};

std::vector<unsigned char> bits(int n)                   // a descriptor with the first n bits set
{
    std::vector<unsigned char> d(32, 0);
    for (int b = 0; b < n; b++) d[b / 8] |= (unsigned char)(0x80 >> (b % 8));
    return d;
}

template <class T> T *upload(const std::vector<T> &v)
{
    T *p = nullptr;
    if (jsorb_mem_alloc_device((v.size() ? v.size() : 1) * sizeof(T), (void **)&p) != JSORB_OK || (v.size() && jsorb_mem_h2d(p, v.data(), v.size() * sizeof(T)) != JSORB_OK))
        throw std::runtime_error("upload failed");
    return p;
}

} // namespace

int main()
{
    jsorb_fuse_params prm{};
    prm.th = 3.0f; prm.th_low = 50; prm.check_reprojection = 1;
    prm.fx = prm.fy = 256.0f; prm.cx = 160.0f; prm.cy = 120.0f; prm.bf = 32.0f;
    prm.min_x = 0.0f; prm.max_x = 320.0f; prm.min_y = 0.0f; prm.max_y = 240.0f; prm.cols = 64; prm.rows = 48;
    prm.inv_w = 64.0f / 320.0f; prm.inv_h = 48.0f / 240.0f;
    prm.log_scale_factor = std::log(1.2f); prm.n_levels = 8;
    for (int l = 0; l < 8; l++) { prm.scale_factor[l] = l ? prm.scale_factor[l - 1] * 1.2f : 1.0f; prm.inv_level_sigma2[l] = 1.0f / (prm.scale_factor[l] * prm.scale_factor[l]); }

    // every keyframe at the identity: point r (r < 12: the current keyframe's) sits at depth 4 behind pixel (40 + 20 r, 60); rows 12.. are the
    // neighbours' own points at the same pixels
    auto pixel = [](int i) { return 40.0f + 20.0f * (float)i; };
    std::vector<jsorb_map_point_record> rec(N_ROWS);
    std::vector<int32_t> all_rows(N_ROWS);
    std::vector<float> pf[9];
    for (int r = 0; r < N_ROWS; r++) {
        const float x = (pixel(r % KP) - 160.0f) * 4.0f / 256.0f, y = (60.0f - 120.0f) * 4.0f / 256.0f, z = 4.0f, dist = std::sqrt(x * x + y * y + z * z);
        const float maxd = dist / std::sqrt(1.2f);           // predicts level 0
        const float v[9] = {x, y, z, 0.0f, 0.0f, 1.0f, maxd, 1.2f * maxd, 0.1f * maxd};
        jsorb_map_point_record &m = rec[r];
        m = jsorb_map_point_record{};
        m.P[0] = x; m.P[1] = y; m.P[2] = z; m.Pn[0] = 0.0f; m.Pn[1] = 0.0f; m.Pn[2] = 1.0f;
        m.MaxDistance = maxd; m.invariance_maxDistance = v[7]; m.invariance_minDistance = v[8]; m.bad = r == 20;
        all_rows[r] = r;
        for (int k = 0; k < 9; k++) pf[k].push_back(k == 7 ? v[8] : k == 8 ? v[7] : v[k]);      // jsorb_fuse's order: max_distance, min_dist_inv, max_dist_inv
    }
    Twin tw;
    tw.mps.assign(S, {}); tw.reg.assign(S, {}); tw.kdesc.assign(S, {});
    tw.bad.assign(N_ROWS, 0); tw.bad[20] = 1;
    tw.desc.assign(32 * N_ROWS, 0);
    for (int s = 0; s < 5; s++) {
        tw.mps[s].assign(KP, -1); tw.reg[s].assign(KP, 0);
        for (int i = 0; i < KP; i++) { const auto d = bits((3 * s + 5 * i) % 40); tw.kdesc[s].insert(tw.kdesc[s].end(), d.begin(), d.end()); }
    }
    auto see = [&](int s, int i, int r) { tw.mps[s][i] = r; tw.reg[s][i] = !tw.bad[r]; };
    for (int i = 0; i < KP - 1; i++) see(CUR, i, i);                       // (the last keypoint of the current keyframe has no point: a NULL list entry)
    for (int i = 0; i < 6; i++) see(4, i, i);                              // points 0-5: two observations
    see(1, 1, 12); see(2, 1, 12); see(3, 1, 12);                           // 12: three observations against point 1's two
    see(1, 7, 13);                                                         // 13: one, as many as point 7
    see(2, 8, 14); see(4, 8, 14); see(1, 8, 15);                           // 14: two against point 8's one; 15 in another neighbour
    see(3, 3, 20);                                                         // a bad point in a slot
    see(2, 10, 16); see(3, 10, 16); see(4, 10, 16);
    see(2, 11, 23);                                                        // 23: behind the pixel of that last keypoint - the second direction adds it there

    jsorb::KeyframeMatcher matcher(0);
    jsorb::KeyframeGraph graph(S, 256, 8);
    jsorb::MapPointTable table(N_ROWS);
    table.scatter(all_rows, rec, matcher.stream());
    table.set_descriptors(0, N_ROWS, tw.desc.data());
    jsorb::KeyframeKeypoints kp(graph, false);
    jsorb::Covisibility cov(S, 16);
    std::vector<float> kx(KP), ky(KP, 60.0f);
    for (int i = 0; i < KP; i++) kx[i] = pixel(i);
    for (int s = 0; s < 5; s++) {
        graph.set_keyframe(s, tw.mps[s], 100 + s, jsorb::KeyframeGraph::GOOD, &tw.reg[s]);
        kp.set_keyframe(graph, s, kx, ky, std::vector<int32_t>(KP, 0), nullptr, tw.kdesc[s]);
        cov.created(s, s == 4);
    }
    jsorb::FuseState state(graph, table);

    // ---- the twin: one jsorb_fuse per keyframe, the tail on the host ----
    float *dx = upload(kx), *dy = upload(ky);
    int32_t *doct = upload(std::vector<int32_t>(KP, 0));
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
    auto host_fuse = [&](const std::vector<int32_t> &list, const std::vector<int32_t> &targets) {
        for (int A : targets) {
            const int n = (int)list.size();
            std::vector<float> g[9];
            std::vector<unsigned char> gd, skip;
            for (int r : list) {
                for (int k = 0; k < 9; k++) g[k].push_back(pf[k][r]);
                gd.insert(gd.end(), &tw.desc[32 * r], &tw.desc[32 * r] + 32);
                bool in_kf = false;
                for (auto &o : tw.observations(r)) in_kf = in_kf || o.first == A;
                skip.push_back(tw.bad[r] || in_kf);
            }
            float *d[9];
            for (int k = 0; k < 9; k++) d[k] = upload(g[k]);
            unsigned char *dd = upload(gd), *ds = upload(skip), *dk = upload(tw.kdesc[A]);
            const int32_t ks[2] = {0, KP};
            std::vector<int32_t> bi(n, -1), bd(n, -1);
            int matched = 0;
            if (jsorb_fuse(matcher.handle(), &prm, n, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], dd, 1, ks, dx, dy, doct, nullptr, dk, I, zero, zero, ds,
                           bi.data(), bd.data(), &matched) != JSORB_OK)
                throw std::runtime_error(jsorb_keyframe_matcher_last_error(matcher.handle()));
            for (int k = 0; k < 9; k++) jsorb_mem_free_device(d[k]);
            jsorb_mem_free_device(dd); jsorb_mem_free_device(ds); jsorb_mem_free_device(dk);
            for (int i = 0; i < n; i++) {
                const int r = list[i];
                bool in_kf = false;
                for (auto &o : tw.observations(r)) in_kf = in_kf || o.first == A;
                if (tw.bad[r] || in_kf || bi[i] < 0) continue;                   // the head test on the live map
                const int q = tw.mps[A][bi[i]];
                if (q < 0) { tw.mps[A][bi[i]] = r; tw.reg[A][bi[i]] = 1; tw.events.push_back({3, r, A, bi[i]}); }
                else if (!tw.bad[q]) { if (tw.observations(q).size() > tw.observations(r).size()) tw.replace(r, q); else tw.replace(q, r); }
            }
        }
    };
    auto neighbour_rows = [&]() {
        std::vector<int32_t> rows;
        for (int s = 1; s <= 3; s++)
            for (int r : tw.mps[s])
                if (r >= 0 && !tw.bad[r] && std::find(rows.begin(), rows.end(), r) == rows.end()) rows.push_back(r);
        return rows;
    };
    const std::vector<int32_t> listA(tw.mps[CUR]), targetsA = {1, 2, 3};
    host_fuse(listA, targetsA);
    const std::vector<int32_t> listB = neighbour_rows();
    host_fuse(listB, {CUR});

    // ---- the device: two calls ----
    std::vector<float> R3, z9(9, 0.0f);
    for (int t = 0; t < 3; t++) R3.insert(R3.end(), I, I + 9);
    const jsorb::FusePoses poses{R3.data(), z9.data(), z9.data()};
    jsorb::FusedMap a, b;
    const int fusedA = Jetson_SLAM::FuseMap(matcher, prm, graph, table, kp, state, listA, targetsA, poses, a);
    const int fusedB = Jetson_SLAM::FuseMap(matcher, prm, graph, table, kp, state, listB, {CUR}, poses, b);
    jsorb::UpdatedConnections updated;
    Jetson_SLAM::UpdateConnections(matcher, graph, table, cov, {0, 1, 2, 3, 4}, updated);

    // ---- compare ----
    std::vector<std::array<int32_t, 4>> ev(a.events);
    ev.insert(ev.end(), b.events.begin(), b.events.end());
    bool ok = true;
    auto expect = [&](bool v, const char *what) { if (!v) { std::printf("differs: %s\n", what); ok = false; } };
    expect(ev == tw.events, "the event log");
    expect(fusedA > 0 && fusedB > 0 && a.counts[1] > 0 && a.counts[2] > 0 && a.counts[3] > 0 && b.counts[2] > 0, "every branch taken");
    const jsorb_keyframe_graph g = graph.view();
    const jsorb_map_point_table t = table.view();
    for (int s = 0; s < 5; s++) {
        std::vector<int32_t> pool(KP);
        std::vector<unsigned char> reg(KP);
        jsorb_mem_d2h(pool.data(), g.point_pool + graph.point_offset(s), KP * sizeof(int32_t));
        jsorb_mem_d2h(reg.data(), g.registered + graph.point_offset(s), KP);
        expect(pool == tw.mps[s] && reg == tw.reg[s], "a keyframe's slots");
    }
    std::vector<unsigned char> bad(N_ROWS), desc(32 * N_ROWS);
    jsorb_mem_d2h(bad.data(), t.bad, N_ROWS);
    jsorb_mem_d2h(desc.data(), t.desc, 32 * N_ROWS);
    expect(bad == tw.bad, "the bad flags");
    for (int r = 0; r < N_ROWS; r++)
        if (!tw.bad[r]) expect(std::equal(&desc[32 * r], &desc[32 * r] + 32, &tw.desc[32 * r]), "a descriptor");
    // the covisibility graph: the same call over the twin's map uploaded afresh
    jsorb::KeyframeGraph graph2(S, 256, 8);
    jsorb::MapPointTable table2(N_ROWS);
    for (int r = 0; r < N_ROWS; r++) rec[r].bad = tw.bad[r];
    table2.scatter(all_rows, rec, matcher.stream());
    jsorb::Covisibility cov2(S, 16);
    for (int s = 0; s < 5; s++) {
        graph2.set_keyframe(s, tw.mps[s], 100 + s, jsorb::KeyframeGraph::GOOD, &tw.reg[s]);
        cov2.created(s, s == 4);
    }
    jsorb::UpdatedConnections updated2;
    Jetson_SLAM::UpdateConnections(matcher, graph2, table2, cov2, {0, 1, 2, 3, 4}, updated2);
    expect(updated.parent == updated2.parent && updated.counts[0] == 5, "UpdateConnections' parents");
    for (int s = 0; s < 5; s++) {
        const jsorb::Covisibility::Slot c1 = cov.copy(s), c2 = cov2.copy(s);
        expect(c1.conn_slot == c2.conn_slot && c1.conn_weight == c2.conn_weight && c1.ord_slot == c2.ord_slot && c1.ord_weight == c2.ord_weight, "the covisibility lists");
    }
    std::printf("direction A: %d fused, %d Replace, %d AddMapPoint; direction B: %d fused, %d Replace, %d AddMapPoint; %zu events\n", fusedA, a.counts[1],
                a.counts[2], fusedB, b.counts[1], b.counts[2], ev.size());
    for (void *p : {(void *)dx, (void *)dy, (void *)doct}) jsorb_mem_free_device(p);
    std::printf(ok ? "ok\n" : "MISMATCH\n");
    return ok ? 0 : 1;
}
