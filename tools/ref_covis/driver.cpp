// tools/ref_covis/driver.cpp - runs worlds of tests/covis_cases.py through the reference's own src/KeyFrame.cpp (compiled unmodified against the
// stand-in headers of this directory) and records every keyframe's map, ordered lists, first-connection flag, parent and children after each
// step.  The keyframes live in ONE array in (order_key, slot) order behind a keyframe that is no slot (it takes mnId 0), so std::map<KeyFrame*,
// ...>'s pointer order is the world's key order.  A step is an update - UpdateConnections() of its slots in order, a slot that is unusable, has
// an invalid run or occurred before in the step being skipped as the contract says - or an erase - SetBadFlag().  Probe derives from KeyFrame
// to read, and to load a world's state into, the protected members.  AUTHORING TOOLING ONLY (tools/ref_covis_goldens.py).
// usage: driver <world.bin> <out.bin>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "KeyFrame.h"

using namespace Jetson_SLAM;

struct Probe : public KeyFrame {
    Probe(Frame &F, Map *m, KeyFrameDatabase *db) : KeyFrame(F, m, db) {}
    void load(bool first, const std::map<KeyFrame *, int> &conn, const std::vector<KeyFrame *> &ord, const std::vector<int> &w)
    {
        mbFirstConnection = first; mConnectedKeyFrameWeights = conn; mvpOrderedConnectedKeyFrames = ord; mvOrderedWeights = w;
    }
    bool first() const { return mbFirstConnection; }
    const std::map<KeyFrame *, int> &conn() const { return mConnectedKeyFrameWeights; }
    const std::vector<KeyFrame *> &ord() const { return mvpOrderedConnectedKeyFrames; }
    const std::vector<int> &ord_w() const { return mvOrderedWeights; }
};

static std::vector<int32_t> read_i32(FILE *f, size_t n)
{
    std::vector<int32_t> v(n);
    if (n && fread(v.data(), 4, n, f) != n) { fprintf(stderr, "short world file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = read_i32(f, 6);
    const int S = hd[0], n_rows = hd[1], pool_len = hd[2], C = hd[3], n_steps = hd[4], n_args = hd[5];
    const std::vector<int32_t> state = read_i32(f, S);
    std::vector<int64_t> key(S);
    if (fread(key.data(), 8, S, f) != (size_t)S) return 2;
    const std::vector<int32_t> off = read_i32(f, S), len = read_i32(f, S), pool = read_i32(f, pool_len), reg = read_i32(f, pool_len), bad = read_i32(f, n_rows),
                               first = read_i32(f, S), conn_len = read_i32(f, S), conn_slot = read_i32(f, (size_t)S * C), conn_w = read_i32(f, (size_t)S * C),
                               ord_len = read_i32(f, S), ord_slot = read_i32(f, (size_t)S * C), ord_w = read_i32(f, (size_t)S * C),
                               kind = read_i32(f, n_steps), start = read_i32(f, n_steps + 1), args = read_i32(f, n_args);
    fclose(f);

    // the array: index 0 is no slot, index 1 + rank the slot of that rank in (key, slot) order
    std::vector<int> by_rank(S), index_of(S);
    for (int s = 0; s < S; s++) by_rank[s] = s;
    std::sort(by_rank.begin(), by_rank.end(), [&](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
    for (int r = 0; r < S; r++) index_of[by_rank[r]] = r + 1;
    static Frame F;
    static Map the_map;
    static KeyFrameDatabase db;
    std::vector<MapPoint> points(n_rows);
    for (int r = 0; r < n_rows; r++) points[r].bad = bad[r] != 0;
    Probe *kf = static_cast<Probe *>(operator new[](sizeof(Probe) * (S + 1)));
    auto run_ok = [&](int s) { return off[s] >= 0 && len[s] >= 0 && (long long)off[s] + len[s] <= pool_len; };
    F.mvpMapPoints.clear();
    new (&kf[0]) Probe(F, &the_map, &db);
    for (int r = 0; r < S; r++) {
        const int s = by_rank[r];
        F.mvpMapPoints.clear();
        if (state[s] != 0 && run_ok(s))
            for (int j = 0; j < len[s]; j++) {
                const int row = pool[off[s] + j];
                F.mvpMapPoints.push_back(row >= 0 && row < n_rows ? &points[row] : nullptr);
            }
        new (&kf[r + 1]) Probe(F, &the_map, &db);
    }
    for (int s = 0; s < S; s++)
        if (state[s] != 0 && run_ok(s))
            for (int j = 0; j < len[s]; j++) {
                const int row = pool[off[s] + j];
                if (row >= 0 && row < n_rows && reg[off[s] + j]) points[row].observations[&kf[index_of[s]]] = j;
            }
    for (int s = 0; s < S; s++) {
        std::map<KeyFrame *, int> conn;
        std::vector<KeyFrame *> ord;
        std::vector<int> w;
        for (int j = 0; j < conn_len[s]; j++) conn[&kf[index_of[conn_slot[(size_t)s * C + j]]]] = conn_w[(size_t)s * C + j];
        for (int j = 0; j < ord_len[s]; j++) { ord.push_back(&kf[index_of[ord_slot[(size_t)s * C + j]]]); w.push_back(ord_w[(size_t)s * C + j]); }
        kf[index_of[s]].load(first[s] != 0, conn, ord, w);
    }
    auto slot_of = [&](KeyFrame *p) { return p && p != &kf[0] ? by_rank[static_cast<Probe *>(p) - kf - 1] : -1; };

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int t = 0; t < n_steps; t++) {
        std::vector<int32_t> parent_out(32, -2);
        if (kind[t] == 0) {
            std::vector<char> seen(S, 0);
            for (int i = start[t]; i < start[t + 1] && i - start[t] < 32; i++) {
                const int s = args[i];
                parent_out[i - start[t]] = -1;
                if (s < 0 || s >= S || state[s] == 0 || !run_ok(s) || seen[s]) continue;
                seen[s] = 1;
                Probe &k = kf[index_of[s]];
                const bool before = k.first();
                k.UpdateConnections();
                if (before && !k.first()) parent_out[i - start[t]] = slot_of(k.GetParent());
            }
        } else {
            Probe &k = kf[index_of[args[start[t]]]];
            if (!k.GetParent()) k.ChangeParent(&kf[0]);          // SetBadFlag reads through mpParent
            k.SetBadFlag();
        }
        std::vector<int32_t> lens(5 * (size_t)S, 0), wide(5 * (size_t)S * C, 0);
        int32_t *cs = wide.data(), *cw = cs + (size_t)S * C, *os = cw + (size_t)S * C, *ow = os + (size_t)S * C, *ch = ow + (size_t)S * C;
        for (int s = 0; s < S; s++) {
            const Probe &k = kf[index_of[s]];
            if ((int)k.conn().size() > C || (int)k.ord().size() > C || k.ord_w().size() < k.ord().size()) {      // (SetBadFlag leaves mvOrderedWeights behind)
                fprintf(stderr, "slot %d: a map or a list does not fit\n", s);
                return 3;
            }
            int j = 0;
            for (auto &kw : k.conn()) { cs[(size_t)s * C + j] = slot_of(kw.first); cw[(size_t)s * C + j] = kw.second; j++; }
            lens[s] = j;
            for (j = 0; j < (int)k.ord().size(); j++) { os[(size_t)s * C + j] = slot_of(k.ord()[j]); ow[(size_t)s * C + j] = k.ord_w()[j]; }
            lens[S + s] = j;
            lens[2 * S + s] = k.first();
            lens[3 * S + s] = slot_of(kf[index_of[s]].GetParent());
            j = 0;
            for (KeyFrame *c : kf[index_of[s]].GetChilds()) {
                if (j < C) ch[(size_t)s * C + j] = slot_of(c);
                j++;
            }
            lens[4 * S + s] = j < C ? j : C;
        }
        fwrite(lens.data(), 4, lens.size(), o);
        fwrite(wide.data(), 4, wide.size(), o);
        fwrite(parent_out.data(), 4, parent_out.size(), o);
    }
    fclose(o);
    return 0;
}
