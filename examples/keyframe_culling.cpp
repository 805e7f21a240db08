// keyframe_culling.cpp - LocalMapping::KeyFrameCulling on the device through the C++ shim, on a small map of its own: four keyframes that see the
// same twenty points as the current keyframe, two children of the first of them, the covisibility graph built by UpdateConnections.  The first
// two of the four are redundant when their turn comes (five, then four observations of every point); once they are gone every point is left
// with three observations and the other two are kept - what the reference's loop does, because SetBadFlag runs inside it.  Printed: the decision
// per candidate, the culled slots and the new parents of the culled keyframes' children.
// Usage: keyframe_culling            (no input: the map is made here)
// Exit status 0: two keyframes culled, the rest kept, the children handed on; 1: anything else.
// Build: g++ -std=c++17 -I include examples/keyframe_culling.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <vector>

#include "jsorb_compat.hpp"

int main()
{
    const int S = 8, n_rows = 64, current = 5;
    jsorb::KeyframeMatcher matcher(0);
    jsorb::KeyframeGraph graph(S, 1024, 64);
    jsorb::MapPointTable table(n_rows);
    jsorb::Covisibility cov(S, 16);
    jsorb::KeyframeViews views(graph, false);    // a monocular map: no depth
    // slot 0: the first keyframe; 1-4: the same twenty points; 5: the current keyframe, which sees everything; 6, 7: children of 1 with points of
    // their own that 5 sees too
    std::vector<std::vector<int32_t>> rows(S);
    for (int r = 0; r < 20; r++)
        for (int s = 1; s <= 5; s++) rows[s].push_back(r);
    for (int r = 20; r < 40; r++) { rows[6].push_back(r); rows[7].push_back(r); rows[5].push_back(r); }
    for (int r = 40; r < 60; r++) { rows[0].push_back(r); rows[5].push_back(r); }
    const int parent[S] = {-1, 0, 1, 2, 3, 4, 1, 1};
    for (int s = 0; s < S; s++) {
        graph.set_keyframe(s, rows[s], 4096 + 64 * s);
        graph.set_parent(s, parent[s]);
        views.set_keyframe_views(graph, s, std::vector<unsigned char>(rows[s].size(), 1), std::vector<unsigned char>(rows[s].size(), 0), nullptr, 40.0f);
        cov.created(s, s == 0);
    }
    jsorb::UpdatedConnections updated;
    Jetson_SLAM::UpdateConnections(matcher, graph, table, cov, {0, 1, 2, 3, 4, 5, 6, 7}, updated);
    jsorb::CullingState state(graph, table);
    for (int r = 0; r < 20; r++) state.set_ref_slot(r, 4);       // (the candidate with the highest key comes first among equal weights)

    jsorb::CulledKeyFrames res;
    const int n_culled = Jetson_SLAM::KeyFrameCulling(matcher, graph, table, cov, views, state, current, true, res, 0);
    for (size_t i = 0; i < res.candidates.size(); i++)
        std::printf("candidate %d: decision %d, %d of %d points redundant\n", res.candidates[i], res.decision[i], res.n_redundant[i], res.n_mps[i]);
    std::printf("culled:");
    for (int32_t s : res.culled) std::printf(" %d", s);
    std::printf("\n");
    for (auto &cp : res.reparent) std::printf("keyframe %d: new parent %d\n", cp.first, cp.second);
    std::printf("mpRefKF of point 0: keyframe %d\n", state.ref_slot(0));

    // the binding's part: the child runs of the touched parents
    bool ok = n_culled == 2 && res.counts[1] + res.counts[2] + res.counts[4] == (int)res.candidates.size();
    for (size_t i = 0; i < res.candidates.size(); i++) {
        const int s = res.candidates[i];
        const bool cluster = s >= 1 && s <= 4;
        int earlier = 0;
        for (size_t j = 0; j < i; j++) earlier += res.candidates[j] >= 1 && res.candidates[j] <= 4;
        const int want = s == 0 ? 3 : cluster && earlier < 2 ? 1 : 0;
        ok = ok && res.decision[i] == want;
    }
    ok = ok && !res.reparent.empty() && state.ref_slot(0) != 4;
    std::printf(ok ? "ok\n" : "MISMATCH\n");
    return ok ? 0 : 1;
}
