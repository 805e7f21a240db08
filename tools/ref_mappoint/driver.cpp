// driver.cpp - runs the reference's own MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:273-338, compiled unmodified against the
// reference's include/MapPoint.h) over a WORLD of tests/distinct_cases.py.  AUTHORING TOOLING ONLY (tools/ref_mappoint_goldens.py builds and runs it
// where the reference tree is present; nothing compiled from it is committed).
// The keyframes live in ONE array, so the pointer order of std::map<KeyFrame*, size_t> is the array order.  Every point gets all its observations
// through AddObservation, those in bad keyframes included: the skip of :296 is the reference's.
// Usage: driver in.bin out.bin
//   in.bin   int32: K, R, P, O; kf_start[K + 1]; kf_bad[K]; obs_start[P + 1]; obs_kf[O]; obs_idx[O]; then R x 32 descriptor bytes
//   out.bin  per point: one byte "GetDescriptor() is not empty", then 32 descriptor bytes (zeros when it is empty)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "MapPoint.h"

namespace Jetson_SLAM {

KeyFrame::KeyFrame() : mnId(0), mnFrameId(0), N(0), bad(false) {}
bool KeyFrame::isBad() { return bad; }
cv::Mat KeyFrame::GetCameraCenter() { return Ow.clone(); }
void KeyFrame::EraseMapPointMatch(const size_t &) {}
void KeyFrame::ReplaceMapPointMatch(const size_t &, MapPoint *) {}
void KeyFrame::AddMapPoint(MapPoint *, const size_t &) {}
Frame::Frame() : mnId(0), N(0) {}
cv::Mat Frame::GetCameraCenter() { return cv::Mat::zeros(3, 1, CV_32F); }

}  // namespace Jetson_SLAM

using namespace Jetson_SLAM;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t head[4];
    if (!f || fread(head, 4, 4, f) != 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int K = head[0], R = head[1], P = head[2], O = head[3];
    std::vector<int32_t> kf_start(K + 1), kf_bad(K), obs_start(P + 1), obs_kf(O), obs_idx(O);
    std::vector<unsigned char> desc((size_t)R * 32);
    bool ok = fread(kf_start.data(), 4, K + 1, f) == (size_t)K + 1 && fread(kf_bad.data(), 4, K, f) == (size_t)K &&
              fread(obs_start.data(), 4, P + 1, f) == (size_t)P + 1 && fread(obs_kf.data(), 4, O, f) == (size_t)O &&
              fread(obs_idx.data(), 4, O, f) == (size_t)O && fread(desc.data(), 32, R, f) == (size_t)R;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<KeyFrame> kfs(K);                  // one array: &kfs[a] < &kfs[b] iff a < b
    for (int k = 0; k < K; k++) {
        KeyFrame &kf = kfs[k];
        kf.mnId = kf.mnFrameId = k;
        kf.bad = kf_bad[k] != 0;
        kf.N = kf_start[k + 1] - kf_start[k];
        kf.mDescriptors = cv::Mat(kf.N, 32, CV_8U);
        for (int i = 0; i < kf.N; i++) memcpy(kf.mDescriptors.ptr<unsigned char>(i), &desc[32 * (size_t)(kf_start[k] + i)], 32);
        kf.mvuRight.assign(kf.N, -1.0f);
        kf.Ow = cv::Mat::zeros(3, 1, CV_32F);
    }
    Map map;
    std::vector<unsigned char> out;
    for (int p = 0; p < P; p++) {
        MapPoint mp(cv::Mat::zeros(3, 1, CV_32F), &kfs[0], &map);
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) mp.AddObservation(&kfs[obs_kf[o]], (size_t)obs_idx[o]);
        mp.ComputeDistinctiveDescriptors();
        cv::Mat d = mp.GetDescriptor();
        out.push_back(d.empty() ? 0 : 1);
        for (int b = 0; b < 32; b++) out.push_back(d.empty() ? 0 : d.ptr<unsigned char>(0)[b]);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    return 0;
}
