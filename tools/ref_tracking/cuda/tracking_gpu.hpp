/*
 * A stand-in for the reference's include/cuda/tracking_gpu.hpp and include/cuda/synced_mem_holder.hpp, for tools/ref_tracking: STATIC_MEM_IS_IN is
 * defined, as the reference's header defines it, so that Tracking::SearchLocalPoints takes its SyncedMem branch; SyncedMem<T> is a host vector, as
 * in oracle/ref_matcher/cuda/orb_matcher.hpp; the K16 launcher is defined in driver.cpp, where it records its arguments and forwards to
 * orc_is_in_frustum of oracle/jsorb_oracle.c.
 */
#ifndef JSORB_REF_TRACKING_TRACKING_GPU_HPP
#define JSORB_REF_TRACKING_TRACKING_GPU_HPP

#include <vector>

#define STATIC_MEM_IS_IN

/* resize keeps what the buffer held and never shrinks; cpu and gpu side are one host vector, copies and stream waits do nothing */
template <typename T> class SyncedMem {
public:
    SyncedMem() : count_(0) {}
    void resize(int count) {
        count_ = count;
        if ((int)buf_.size() < count + 1)
            buf_.resize((size_t)count + 1);
    }
    T *cpu_data() { return buf_.data(); }
    T *gpu_data() { return buf_.data(); }
    void to_cpu() {}
    void to_gpu() {}
    void to_cpu_async() {}
    void to_gpu_async() {}
    void sync_stream() {}
    int count_;

private:
    std::vector<T> buf_;
};

namespace tracking_cuda {

void compute_isInFrustum_GPU(int n_points, float *Px, float *Py, float *Pz, float *Pnx, float *Pny, float *Pnz, float *MaxDistance,
                             float *invariance_maxDistance, float *invariance_minDistance, float *Rcw, float *tcw, float *Ow, float &fx, float &fy,
                             float &cx, float &cy, int &minX, int &maxX, int &minY, int &maxY, int &nScaleLevels, float &logScaleFactor,
                             float &viewCosAngle, float *invz, float *u, float *v, int *predictedlevel, float *viewCos, unsigned char *is_infrustum);

}  // namespace tracking_cuda

#endif
