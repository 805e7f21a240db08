// update_connections.cpp - the covisibility graph kept on the device through the C++ shim, next to a host loop over std::map, on a small map of
// its own: (1) LocalMapping::ProcessNewKeyFrame's UpdateConnections for a new keyframe (LocalMapping.cpp:170), (2) a LoopClosing::CorrectLoop-
// shaped run - several keyframes whose points changed, updated one after the other in ONE call (LoopClosing.cpp:437) -, (3) a SetBadFlag
// (KeyFrame.cpp:470-481).  After each stage every keyframe's map, ordered list and weights on the device are compared with the host loop's, and
// so are the parents the first connections give.
// Usage: update_connections            (no input: the map is made here)
// Exit status 0: the device and the host loop agree at every stage; 1: they differ.
// Build: g++ -std=c++17 -I include examples/update_connections.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "jsorb_compat.hpp"

static unsigned rnd_state = 2468u;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

struct KeyFrame;
struct MapPoint {
    int row = 0;
    bool bad = false;
    std::map<KeyFrame *, size_t> observations;
};
struct KeyFrame {
    int slot = 0;
    bool first_connection = true;
    KeyFrame *parent = nullptr;
    std::vector<MapPoint *> points;
    std::map<KeyFrame *, int> weights;
    std::vector<KeyFrame *> ordered;
    std::vector<int> ordered_weights;

    void sort_all()
    {
        std::vector<std::pair<int, KeyFrame *>> v;
        for (auto &kw : weights) v.push_back({kw.second, kw.first});
        set_ordered(v);
    }
    void set_ordered(std::vector<std::pair<int, KeyFrame *>> v)
    {
        std::sort(v.begin(), v.end());
        ordered.clear(); ordered_weights.clear();
        for (size_t i = v.size(); i-- > 0;) { ordered.push_back(v[i].second); ordered_weights.push_back(v[i].first); }
    }
    void add_connection(KeyFrame *kf, int w)
    {
        auto it = weights.find(kf);
        if (it != weights.end() && it->second == w) return;      // nothing changes, the list keeps its form
        weights[kf] = w;
        sort_all();
    }
    void update_connections()
    {
        std::map<KeyFrame *, int> counter;
        for (MapPoint *p : points) {
            if (!p || p->bad) continue;
            for (auto &o : p->observations)
                if (o.first != this) counter[o.first]++;
        }
        if (counter.empty()) return;
        int best = 0;
        KeyFrame *best_kf = nullptr;
        std::vector<std::pair<int, KeyFrame *>> kept;
        for (auto &c : counter) {
            if (c.second > best) { best = c.second; best_kf = c.first; }
            if (c.second >= 15) { kept.push_back({c.second, c.first}); c.first->add_connection(this, c.second); }
        }
        if (kept.empty()) { kept.push_back({best, best_kf}); best_kf->add_connection(this, best); }
        weights = counter;
        set_ordered(kept);
        if (first_connection && slot != 0) { parent = ordered.front(); first_connection = false; }
    }
    void erase_connections()
    {
        for (auto &kw : weights)
            if (kw.first->weights.erase(this)) kw.first->sort_all();
        weights.clear(); ordered.clear(); ordered_weights.clear();
    }
};

static const int N_KF = 20, N_ROWS = 420, PER_KF = 60, STEP = 15;

static void upload(jsorb::KeyframeGraph &graph, KeyFrame &kf)
{
    std::vector<int32_t> rows;
    std::vector<unsigned char> reg;
    for (MapPoint *p : kf.points) {
        rows.push_back(p ? p->row : -1);
        reg.push_back(p && p->observations.count(&kf) ? 1 : 0);
    }
    graph.set_keyframe(kf.slot, rows, (int64_t)(intptr_t)&kf, jsorb::KeyframeGraph::GOOD, &reg);
}

static bool same(const jsorb::Covisibility &cov, std::vector<KeyFrame> &kfs, const char *stage)
{
    for (KeyFrame &kf : kfs) {
        const jsorb::Covisibility::Slot s = cov.copy(kf.slot);
        std::vector<int32_t> cs, cw, os, ow(kf.ordered_weights.begin(), kf.ordered_weights.end());
        for (auto &kw : kf.weights) { cs.push_back(kw.first->slot); cw.push_back(kw.second); }
        for (KeyFrame *o : kf.ordered) os.push_back(o->slot);
        if (cs != s.conn_slot || cw != s.conn_weight || os != s.ord_slot || ow != s.ord_weight) {
            fprintf(stderr, "%s: keyframe %d differs (map %zu/%zu, list %zu/%zu)\n", stage, kf.slot, cs.size(), s.conn_slot.size(), os.size(), s.ord_slot.size());
            return false;
        }
        if (Jetson_SLAM::GetBestCovisibilityKeyFrames(cov, kf.slot, 3) != std::vector<int32_t>(os.begin(), os.begin() + std::min<size_t>(3, os.size()))) return false;
    }
    return true;
}

int main()
{
    try {
        std::vector<MapPoint> mps(N_ROWS);
        std::vector<KeyFrame> kfs(N_KF);         // (their addresses ascend with the slot: std::map's order is the slot order here)
        std::vector<jsorb_map_point_record> rec(N_ROWS);
        std::vector<int32_t> all_rows(N_ROWS);
        for (int r = 0; r < N_ROWS; r++) {
            mps[r].row = r;
            mps[r].bad = r % 23 == 0;
            rec[r] = jsorb_map_point_record{};
            rec[r].bad = mps[r].bad;
            all_rows[r] = r;
        }
        for (int k = 0; k < N_KF; k++) {
            kfs[k].slot = k;
            for (int j = 0; j < PER_KF; j++) {
                MapPoint *p = rnd() % 6 == 0 ? nullptr : &mps[(k * STEP + j) % N_ROWS];
                kfs[k].points.push_back(p);
                if (p && k + 1 < N_KF) p->observations[&kfs[k]] = j;     // (the last keyframe is the new one of stage 1)
            }
        }
        jsorb::KeyframeMatcher matcher;
        jsorb::MapPointTable table(N_ROWS);
        table.scatter(all_rows, rec, matcher.stream());
        jsorb::KeyframeGraph graph(32, N_KF * PER_KF + 256, 16);
        jsorb::Covisibility cov(32, 32);
        jsorb::UpdatedConnections res;
        bool ok = true;

        // the map so far: keyframes 0 .. N_KF-2, each updated when it was made
        std::vector<int32_t> slots;
        for (int k = 0; k + 1 < N_KF; k++) {
            upload(graph, kfs[k]);
            cov.created(k, k == 0);
            slots.push_back(k);
        }
        for (int k = 0; k + 1 < N_KF; k++) kfs[k].update_connections();
        Jetson_SLAM::UpdateConnections(matcher, graph, table, cov, slots, res);
        for (int k = 0; k + 1 < N_KF; k++) ok = ok && res.parent[k] == (kfs[k].parent ? kfs[k].parent->slot : -1);
        ok = ok && same(cov, kfs, "the map so far");

        // (1) ProcessNewKeyFrame: the new keyframe's points gain their observation, then its UpdateConnections
        KeyFrame &fresh = kfs[N_KF - 1];
        for (size_t j = 0; j < fresh.points.size(); j++)
            if (fresh.points[j]) fresh.points[j]->observations[&fresh] = j;
        upload(graph, fresh);
        cov.created(fresh.slot);
        fresh.update_connections();
        Jetson_SLAM::UpdateConnections(matcher, graph, table, cov, {fresh.slot}, res);
        ok = ok && res.parent[0] == fresh.parent->slot && res.counts[0] == 1 && same(cov, kfs, "ProcessNewKeyFrame");
        const int parent_of_new = res.parent[0];

        // (2) CorrectLoop: the loop's keyframes take over points of the old side, then each is updated, in order, in one call
        slots.clear();
        for (int k = 3; k <= 8; k++) {
            for (int j = 0; j < 20; j++) {
                MapPoint *p = &mps[(15 * STEP + 2 * j + k) % N_ROWS];
                if (p->observations.count(&kfs[k])) continue;
                MapPoint *&place = kfs[k].points[40 + j];
                if (place) place->observations.erase(&kfs[k]);
                place = p;
                p->observations[&kfs[k]] = 40 + j;
            }
            upload(graph, kfs[k]);
            slots.push_back(k);
        }
        for (int k : slots) kfs[k].update_connections();
        Jetson_SLAM::UpdateConnections(matcher, graph, table, cov, slots, res);
        ok = ok && res.counts[0] == (int)slots.size() && res.counts[4] > 0 && same(cov, kfs, "CorrectLoop");

        // (3) SetBadFlag of keyframe 6: its neighbours forget it, its own map and lists are empty
        const int held_host = (int)std::count_if(kfs[6].weights.begin(), kfs[6].weights.end(), [&](const std::pair<KeyFrame *const, int> &kw) { return kw.first->weights.count(&kfs[6]) > 0; });
        kfs[6].erase_connections();
        const int held = Jetson_SLAM::EraseConnections(matcher, graph, cov, 6);
        graph.set_state(6, jsorb::KeyframeGraph::BAD);
        ok = ok && held == held_host && same(cov, kfs, "SetBadFlag") && Jetson_SLAM::GetConnectedKeyFrames(cov, 6).empty() &&
             Jetson_SLAM::GetWeight(cov, 7, 6) == 0 && Jetson_SLAM::GetWeight(cov, 7, 8) == kfs[7].weights[&kfs[8]];

        printf("%s keyframes=%d parent_of_new=%d loop_resorted=%d erased_from=%d\n", ok ? "ok" : "MISMATCH", N_KF, parent_of_new, res.counts[4], held);
        return ok && held > 0 ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
