// distinct_host_loop.cpp - the host loop of examples/search_in_neighbors.cpp / examples/update_map_points.cpp (MapPoint.cpp:273-338: pairwise Hamming
// distances, a sort per observation, the first smallest lower median) over the inputs of tools/distinct_bench.py, timed: the scale the device call's
// time stands against.  Host only.
// Usage: distinct_host_loop in.bin reps        in.bin: int32 P, O, R; obs_start[P + 1]; obs_row[O]; R x 32 descriptor bytes
// Prints: host_loop_us=<median over reps of one pass over all points> checksum=<sum of the winners' rows>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin reps\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t head[3];
    if (!f || fread(head, 4, 3, f) != 3) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int P = head[0], O = head[1], R = head[2], reps = atoi(argv[2]);
    std::vector<int32_t> obs_start(P + 1), obs_row(O);
    std::vector<unsigned char> desc((size_t)R * 32), out((size_t)P * 32);
    if (fread(obs_start.data(), 4, P + 1, f) != (size_t)P + 1 || fread(obs_row.data(), 4, O, f) != (size_t)O || fread(desc.data(), 32, R, f) != (size_t)R) return 2;
    fclose(f);
    std::vector<double> spans;
    long long checksum = 0;
    for (int rep = 0; rep < reps; rep++) {
        checksum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int p = 0; p < P; p++) {
            const int s = obs_start[p], N = obs_start[p + 1] - s;
            if (N == 0) continue;
            int bestMedian = INT_MAX, best = 0;
            for (int i = 0; i < N; i++) {
                std::vector<int> row(N);
                for (int j = 0; j < N; j++) row[j] = hamming(&desc[32 * (size_t)obs_row[s + i]], &desc[32 * (size_t)obs_row[s + j]]);
                std::sort(row.begin(), row.end());
                const int median = row[(size_t)(0.5 * (double)(N - 1))];
                if (median < bestMedian) { bestMedian = median; best = i; }
            }
            memcpy(&out[32 * (size_t)p], &desc[32 * (size_t)obs_row[s + best]], 32);
            checksum += obs_row[s + best];
        }
        spans.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(spans.begin(), spans.end());
    printf("host_loop_us=%.1f checksum=%lld\n", spans[spans.size() / 2], checksum);
    return 0;
}
