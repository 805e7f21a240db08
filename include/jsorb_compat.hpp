// jsorb_compat.hpp - header-only C++ shim that recreates the reference's GPU-side interface on top of the C ABI (include/jsorb.h),
// so that Frame / Tracking / ORBmatcher keep compiling against the same names.  It stands in for these reference headers:
//
//   include/cuda/synced_mem_holder.hpp:10-65   orb_cuda::SyncedMem<T>     every member: count_, capacity_, cpu_data_, gpu_data_, pitch_,
//                                                                         cu_stream_, resize, resize_pitched, cpu_data, gpu_data,
//                                                                         to_cpu/to_gpu (+count, +async, +stream), sync_stream, set_zero_*
//   include/cuda/orb_gpu.hpp:22-250            orb_cuda::ORB_GPU          ctor argument order, extract(), ORB_compute_stereo_match(),
//                                                                         height_, width_, scale_, inv_scale_, image_ (what Frame.cpp:780-803 touches)
//   include/cuda/orb_matcher.hpp:12-24         orb_cuda::ORB_Search_by_projection_project_on_frame, ORB_compute_distances
//   include/cuda/tracking_gpu.hpp:14-31        tracking_cuda::compute_isInFrustum_GPU
//   include/ORBextractor.h:21-93               Jetson_SLAM::ORBExtractor  ctor argument order, extract(), get_* tables, orb_gpu_
//
// plus three helpers that are the bodies of Frame.cpp:119-196 (UnpackFrame), :463-479 (AssignFeaturesToGrid) and a free-function form of
// Frame::ComputeStereoMatches.  No HIP / CUDA / OpenCV header is needed by the consumer: all device work goes through the ABI.
// Define JSORB_WITH_OPENCV before including to get the cv::Mat / cv::KeyPoint overloads (the exact reference signatures) and mask
// loading through cv::imread; without it masks are decoded by libjsorb itself (PNG, binary PGM / PPM: jsorb_read_mask_image).
#ifndef JSORB_COMPAT_HPP
#define JSORB_COMPAT_HPP

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <string>
#include <array>
#include <vector>

#include "jsorb.h"

#ifdef JSORB_WITH_OPENCV
#include <opencv2/core.hpp>
#include <opencv2/imgcodecs.hpp>
#include <opencv2/imgproc.hpp>
#endif

// The reference's host code names these CUDA types (SyncedMem::cu_stream_, to_cpu_async(cudaStream_t&)); they are opaque here.
#ifndef JSORB_NO_CUDA_TYPEDEFS
typedef void *cudaStream_t;
typedef int cudaError_t;
#endif

namespace orb_cuda {

// Buffer pairs (pinned host + device) released by SyncedMem objects are parked here and handed to the next object that asks for the same
// capacity.  The reference's Frame holds four SyncedMem members (Frame.h:234-237, the static variant is commented out), so EVERY frame
// runs cudaMallocHost + cudaMalloc four times and frees them again; here a steady-state frame allocates nothing.  Per process, bounded,
// guarded by a mutex (the two extractor threads of a stereo frame release / acquire concurrently).
namespace detail {
struct SyncedBufferCache {
    struct Entry { size_t bytes; void *cpu, *gpu; };
    std::mutex mu;
    std::vector<Entry> free_list;
    std::vector<cudaStream_t> free_streams;         // creating and destroying a HIP stream costs milliseconds: the private streams are recycled too
    static SyncedBufferCache &get() { static SyncedBufferCache c; return c; }
    int take_stream(cudaStream_t *st)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!free_streams.empty()) { *st = free_streams.back(); free_streams.pop_back(); return JSORB_OK; }
        }
        return jsorb_mem_stream_create(st);
    }
    void give_stream(cudaStream_t st, bool used)
    {
        if (!st) return;
        if (used) jsorb_mem_stream_sync(st);       // a stream that never carried work needs no wait (hipStreamSynchronize is ~5 us, four per Frame)
        {
            std::lock_guard<std::mutex> lk(mu);
            if (free_streams.size() < 64) { free_streams.push_back(st); return; }
        }
        jsorb_mem_stream_destroy(st);
    }
    bool take(size_t bytes, void **cpu, void **gpu)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < free_list.size(); i++)
            if (free_list[i].bytes == bytes) {
                *cpu = free_list[i].cpu; *gpu = free_list[i].gpu;
                free_list[i] = free_list.back(); free_list.pop_back();
                return true;
            }
        return false;
    }
    void give(size_t bytes, void *cpu, void *gpu)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (cpu && gpu && free_list.size() < 32) { free_list.push_back(Entry{bytes, cpu, gpu}); return; }
        }
        if (cpu) jsorb_mem_free_host(cpu);
        if (gpu) jsorb_mem_free_device(gpu);
    }
    ~SyncedBufferCache()
    {
        for (auto &e : free_list) { jsorb_mem_free_host(e.cpu); jsorb_mem_free_device(e.gpu); }
        for (auto st : free_streams) jsorb_mem_stream_destroy(st);
    }
};
}

// orb_cuda::SyncedMem<T> (synced_mem_holder.hpp:10-65, synced_mem_holder.cpp:8-199): a pinned host buffer + a device buffer of
// capacity_ elements and a private stream.  Same semantics: resize() grows only and never clears; the to_* calls copy count_
// (or the given count) elements; the *_async forms run on cu_stream_ (or the given stream) and sync_stream() waits for cu_stream_.
// Errors are recorded in cu_error_ and otherwise ignored, as in the reference (every method there is void).
// COPIES: the reference declares no copy operations, so a copied SyncedMem there aliases the original's buffers and stream (and frees
// them twice).  Frame is copied and assigned all the time (Tracking.cpp:292/336/364/366: mCurrentFrame = Frame(...); Frame(mCurrentFrame)),
// so the copy operations exist here, with the reference's aliasing made safe: a copy SHARES the buffers and the stream with the
// original (a reference count decides who frees); an object that has to grow while it shares leaves the old buffers to the others.
template <typename Dtype>
class SyncedMem {
    // shared by every copy of a SyncedMem: the buffers, the private stream, and what is known about them - whether the host side is current
    // (host_fresh: a copy that writes the device side invalidates it for ALL aliases; round-3 review) and whether work the library cannot see
    // may still be using the device buffer (foreign: the caller took gpu_data() or queued a copy on a stream of its own)
    struct Owner {
        void *cpu = nullptr, *gpu = nullptr; cudaStream_t stream = nullptr; size_t bytes = 0; bool pitched = false;
        std::atomic<bool> stream_used{false}, host_fresh{false}, foreign{false};
        std::atomic<int> refs{1};
    };

public:
    SyncedMem() : count_(0), capacity_(0), cpu_data_(nullptr), gpu_data_(nullptr), pitch_(0), cu_stream_(nullptr), cu_error_(0), own_(new Owner)
    {
        cu_error_ = detail::SyncedBufferCache::get().take_stream(&cu_stream_);
        own_->stream = cu_stream_;
    }
    ~SyncedMem() { release(); }
    SyncedMem(const SyncedMem &o)
        : count_(o.count_), capacity_(o.capacity_), cpu_data_(o.cpu_data_), gpu_data_(o.gpu_data_), pitch_(o.pitch_), cu_stream_(o.cu_stream_),
          cu_error_(o.cu_error_), own_(o.own_)
    {
        if (own_) own_->refs.fetch_add(1);
    }
    SyncedMem &operator=(const SyncedMem &o)
    {
        if (this == &o) return *this;
        if (o.own_) o.own_->refs.fetch_add(1);
        release();
        count_ = o.count_; capacity_ = o.capacity_; cpu_data_ = o.cpu_data_; gpu_data_ = o.gpu_data_; pitch_ = o.pitch_; cu_stream_ = o.cu_stream_;
        cu_error_ = o.cu_error_; own_ = o.own_;
        return *this;
    }
    SyncedMem(SyncedMem &&o) noexcept
        : count_(o.count_), capacity_(o.capacity_), cpu_data_(o.cpu_data_), gpu_data_(o.gpu_data_), pitch_(o.pitch_), cu_stream_(o.cu_stream_),
          cu_error_(o.cu_error_), own_(o.own_)
    {
        o.count_ = o.capacity_ = 0; o.cpu_data_ = nullptr; o.gpu_data_ = nullptr; o.cu_stream_ = nullptr; o.own_ = nullptr;
    }
    SyncedMem &operator=(SyncedMem &&o) noexcept
    {
        if (this == &o) return *this;
        release();
        count_ = o.count_; capacity_ = o.capacity_; cpu_data_ = o.cpu_data_; gpu_data_ = o.gpu_data_; pitch_ = o.pitch_; cu_stream_ = o.cu_stream_;
        cu_error_ = o.cu_error_; own_ = o.own_;
        o.count_ = o.capacity_ = 0; o.cpu_data_ = nullptr; o.gpu_data_ = nullptr; o.cu_stream_ = nullptr; o.own_ = nullptr;
        return *this;
    }

    void resize(int count)
    {
        count_ = count;
        set_host_fresh(false);
        if (capacity_ < count_) {
            capacity_ = count_;
            fresh_owner();
            const size_t bytes = (size_t)capacity_ * sizeof(Dtype);
            void *c = nullptr, *g = nullptr;
            if (!detail::SyncedBufferCache::get().take(bytes, &c, &g)) {
                note(jsorb_mem_alloc_host(bytes, &c));
                note(jsorb_mem_alloc_device(bytes, &g));
            }
            cpu_data_ = (Dtype *)c; gpu_data_ = (Dtype *)g;
            own_->cpu = c; own_->gpu = g; own_->bytes = bytes; own_->pitched = false;
        }
    }
    void resize_pitched(size_t width, size_t height)
    {
        count_ = (int)(width * height);
        set_host_fresh(false);
        fresh_owner();
        void *c = nullptr, *g = nullptr;
        note(jsorb_mem_alloc_host((size_t)count_ * sizeof(Dtype), &c));
        note(jsorb_mem_alloc_device_pitched(width * sizeof(Dtype), height, &g, &pitch_));
        cpu_data_ = (Dtype *)c; gpu_data_ = (Dtype *)g;
        own_->cpu = c; own_->gpu = g; own_->bytes = 0; own_->pitched = true;
    }

    // the caller may write through either pointer: the other side is no longer known to be current (to_cpu() then copies, as
    // synced_mem_holder.cpp:88-91 always does)
    Dtype *cpu_data() { set_host_fresh(false); return cpu_data_; }
    Dtype *gpu_data() { set_host_fresh(false); if (own_) own_->foreign.store(true); return gpu_data_; }

    void to_cpu(void) { to_cpu(count_); }
    void to_gpu(void) { to_gpu(count_); }
    void to_cpu(int count)
    {
        if (host_fresh() && count <= count_) return;      // ORBExtractor::extract already delivered the host copy with the device copy and nobody has asked for a pointer since
        note(jsorb_mem_d2h(cpu_data_, gpu_data_, (size_t)count * sizeof(Dtype)));
    }
    void to_gpu(int count) { set_host_fresh(false); note(jsorb_mem_h2d(gpu_data_, cpu_data_, (size_t)count * sizeof(Dtype))); }
    void to_cpu_async(void) { to_cpu_async(cu_stream_, count_); }
    void to_gpu_async(void) { to_gpu_async(cu_stream_, count_); }
    void to_cpu_async(cudaStream_t &cu_stream) { to_cpu_async(cu_stream, count_); }
    void to_gpu_async(cudaStream_t &cu_stream) { to_gpu_async(cu_stream, count_); }
    void to_cpu_async(int count) { to_cpu_async(cu_stream_, count); }
    void to_gpu_async(int count) { to_gpu_async(cu_stream_, count); }
    void to_cpu_async(cudaStream_t &cu_stream, int count)
    {
        if (host_fresh() && count <= count_) return;
        mark_stream(cu_stream);
        note(jsorb_mem_d2h_async(cpu_data_, gpu_data_, (size_t)count * sizeof(Dtype), cu_stream));
    }
    void to_gpu_async(cudaStream_t &cu_stream, int count)
    {
        set_host_fresh(false);
        mark_stream(cu_stream);
        note(jsorb_mem_h2d_async(gpu_data_, cpu_data_, (size_t)count * sizeof(Dtype), cu_stream));
    }
    void sync_stream(void) { note(jsorb_mem_stream_sync(cu_stream_)); }
    void set_zero_gpu(void) { set_host_fresh(false); note(jsorb_mem_set_zero(gpu_data_, (size_t)count_ * sizeof(Dtype))); }
    void set_zero_gpu_async(void) { set_host_fresh(false); mark_stream(cu_stream_); note(jsorb_mem_set_zero_async(gpu_data_, (size_t)count_ * sizeof(Dtype), cu_stream_)); }
    void set_zero_cpu(void) { set_host_fresh(false); if (cpu_data_) memset(cpu_data_, 0, (size_t)count_ * sizeof(Dtype)); }

    // public in the reference ("//private:" is commented out there)
    int count_;
    int capacity_;
    Dtype *cpu_data_;
    Dtype *gpu_data_;
    size_t pitch_;
    cudaStream_t cu_stream_;
    cudaError_t cu_error_;

    // set by ORB_GPU::extract when it fills both sides in one go (the four blocking to_cpu() of Frame.cpp:119-122 then cost nothing);
    // cleared by anything that hands out a pointer or moves data.  The flag lives with the shared buffers: every alias sees it.
    void set_host_fresh(bool v) { if (own_) own_->host_fresh.store(v); }
    bool host_fresh() const { return own_ && own_->host_fresh.load(); }

private:
    Owner *own_;
    void note(int rc) { if (rc != JSORB_OK) cu_error_ = rc; }
    // work enqueued on any stream makes the buffers busy until that stream has run: the release paths wait for the private stream only when it was
    // used (work put on a FOREIGN stream is the caller's to synchronise before the object goes away, as in the reference)
    void mark_stream(cudaStream_t st) { if (!own_) return; if (st == own_->stream) own_->stream_used.store(true); else own_->foreign.store(true); }
    // The reference frees with cudaFree / cudaFreeHost, which wait for the whole device; a recycled buffer must not reach its next user while
    // work the library never saw (kernels on gpu_data(), copies on the caller's streams) may still touch it: one device-wide wait then
    static void settle(Owner *o) { if (o->foreign.load()) { jsorb_mem_buffer_sync(o->gpu); o->foreign.store(false); } }      // (the device that owns the buffer, not the thread's current one)
    static void destroy(Owner *o)
    {
        detail::SyncedBufferCache::get().give_stream(o->stream, o->stream_used.load());      // (waits for the stream's work first, if it ever had any)
        if (o->pitched) { if (o->cpu) jsorb_mem_free_host(o->cpu); if (o->gpu) jsorb_mem_free_device(o->gpu); }
        else if (o->cpu || o->gpu) { settle(o); detail::SyncedBufferCache::get().give(o->bytes, o->cpu, o->gpu); }
        delete o;
    }
    void release()
    {
        if (own_ && own_->refs.fetch_sub(1) == 1) destroy(own_);
        own_ = nullptr; cpu_data_ = nullptr; gpu_data_ = nullptr; cu_stream_ = nullptr;
    }
    // before new buffers are attached: sole owner -> the old ones go back to the cache; shared -> they stay with the other objects and
    // this one continues with an owner (and stream) of its own
    void fresh_owner()
    {
        if (own_ && own_->refs.load() == 1) {
            if (own_->pitched) { if (own_->cpu) jsorb_mem_free_host(own_->cpu); if (own_->gpu) jsorb_mem_free_device(own_->gpu); }
            else if (own_->cpu || own_->gpu) {
                if (own_->stream && own_->stream_used.load()) jsorb_mem_stream_sync(own_->stream);
                settle(own_);
                detail::SyncedBufferCache::get().give(own_->bytes, own_->cpu, own_->gpu);
            }
            own_->cpu = own_->gpu = nullptr;
            own_->host_fresh.store(false);
        } else {
            if (own_) own_->refs.fetch_sub(1);
            own_ = new Owner;
            cu_stream_ = nullptr;
            note(detail::SyncedBufferCache::get().take_stream(&cu_stream_));
            own_->stream = cu_stream_;
        }
        cpu_data_ = nullptr; gpu_data_ = nullptr;
    }
};

// orb_cuda::ORB_Search_by_projection_project_on_frame (orb_matcher.hpp:12-18, orb_matcher.cu:62-89): synchronous, device pointers
inline void ORB_Search_by_projection_project_on_frame(int n_points, float *Px_gpu, float *Py_gpu, float *Pz_gpu, float *Rcw_gpu, float *tcw_gpu,
                                                      float &fx, float &fy, float &cx, float &cy, float &minX, float &maxX, float &minY, float &maxY,
                                                      float *u_gpu, float *v_gpu, float *invz_gpu, unsigned char *is_valid_gpu)
{
    if (jsorb_project_points(nullptr, n_points, Px_gpu, Py_gpu, Pz_gpu, Rcw_gpu, tcw_gpu, fx, fy, cx, cy, minX, maxX, minY, maxY, u_gpu, v_gpu, invz_gpu,
                             is_valid_gpu) != JSORB_OK)
        throw std::runtime_error("jsorb_project_points failed");
}
// orb_cuda::ORB_compute_distances (orb_matcher.hpp:20-24, orb_matcher.cu:122-144)
inline void ORB_compute_distances(int n_points, int *idx_left, int *idx_right, unsigned char *descriptor_left, unsigned char *descriptor_right, int *distance)
{
    if (jsorb_hamming_pairs(nullptr, n_points, idx_left, idx_right, descriptor_left, descriptor_right, distance) != JSORB_OK)
        throw std::runtime_error("jsorb_hamming_pairs failed");
}


// orb_cuda::ORB_GPU (include/cuda/orb_gpu.hpp:22-250, src/cuda/orb_gpu.cpp): owns one jsorb handle.  Only the members the reference's
// untouched host code reaches are recreated.
class ORB_GPU {
public:
    // what Frame::ComputeStereoMatches passes as orb_exl.image_ / orb_exr.image_ (Frame.cpp:799-800): the un-blurred pyramid of the last
    // extract, which lives inside the handle
    struct ImagePyramid {
        ORB_GPU *owner = nullptr;
        size_t size() const { return owner ? (size_t)jsorb_n_levels(owner->handle_) : 0; }
        const unsigned char *gpu_data(int level) const { return jsorb_level_image_device(owner->handle_, 0, level, 0); }
    };

    // argument order of orb_gpu.hpp:26-36
    ORB_GPU(int im_height, int im_width, int n_levels, float scale_factor, int FAST_N_MIN, int FAST_N_MAX, int th_FAST_MIN, int th_FAST_MAX, int tile_h,
            int tile_w, bool fixed_multi_scale_tile_size, bool apply_nms_ms, bool nms_ms_mode_gpu, std::string str_mask, int device_id = 0,
            const unsigned char *mask_plane = nullptr, int max_batch = 1)
    {
        std::vector<unsigned char> mask;
        int mask_w = im_width, mask_h = im_height;
        if (!mask_plane && !str_mask.empty()) {
            // orb_gpu.cpp:64-75: cv::imread(str_mask); an unreadable file means "no mask" there (mask.empty() -> all 255)
            int mw = 0, mh = 0;
            bool have = false;
#ifdef JSORB_WITH_OPENCV
            cv::Mat m = cv::imread(str_mask);
            if (!m.empty()) {
                cv::cvtColor(m, m, cv::COLOR_BGR2GRAY);
                mw = m.cols; mh = m.rows;
                mask.resize((size_t)mw * mh);
                for (int y = 0; y < mh; y++) memcpy(&mask[(size_t)y * mw], m.ptr(y), mw);
                have = true;
            }
#else
            // without OpenCV: libjsorb's own decoder (PNG, binary PGM / PPM) with cvtColor(BGR2GRAY)'s 8-bit arithmetic
            int rc = jsorb_read_mask_image(str_mask.c_str(), &mw, &mh, nullptr, 0);
            if (rc == JSORB_OK) {
                mask.resize((size_t)mw * mh);
                rc = jsorb_read_mask_image(str_mask.c_str(), &mw, &mh, mask.data(), mask.size());
            }
            if (rc == JSORB_OK) have = true;
            else if (rc != JSORB_ERR_STATE) throw std::invalid_argument(std::string("jsorb: mask file: ") + jsorb_mask_image_last_error());
#endif
            // the reference resizes whatever size the mask has to EVERY level (level 0 included) with INTER_NN (orb_gpu.cpp:77-81): the mask goes
            // through the ABI at its own size and the library resizes each level from it directly
            if (have) { mask_plane = mask.data(); mask_w = mw; mask_h = mh; }
        }
        jsorb_params p{};
        p.height = im_height; p.width = im_width; p.n_levels = n_levels; p.scale_factor = scale_factor;
        p.fast_n_min = FAST_N_MIN; p.fast_n_max = FAST_N_MAX; p.th_fast_min = th_FAST_MIN; p.th_fast_max = th_FAST_MAX;
        p.tile_h = tile_h; p.tile_w = tile_w; p.fixed_multi_scale_tile_size = fixed_multi_scale_tile_size;
        p.apply_nms_ms = apply_nms_ms; p.nms_ms_mode_gpu = nms_ms_mode_gpu; p.device_id = device_id; p.max_batch = max_batch;
        const int rc = jsorb_create_masked(&p, mask_plane, mask_w, mask_h, &handle_);
        if (rc != JSORB_OK) {
            std::string msg = handle_ ? jsorb_last_error(handle_) : "jsorb_create failed";
            if (handle_) jsorb_destroy(handle_);
            handle_ = nullptr;
            throw std::runtime_error("jsorb_create: " + msg);
        }
        n_levels_ = n_levels;
        for (int i = 0; i < n_levels; i++) {
            int h = 0, w = 0;
            jsorb_level_dims(handle_, i, &h, &w, nullptr);
            height_.push_back(h); width_.push_back(w);
            scale_.push_back(jsorb_scale(handle_, i)); inv_scale_.push_back(jsorb_inv_scale(handle_, i));
        }
        image_.owner = this;
    }
    ORB_GPU(const ORB_GPU &) = delete;
    ORB_GPU &operator=(const ORB_GPU &) = delete;
    ~ORB_GPU() { if (handle_) jsorb_destroy(handle_); }

    // ORB_GPU::extract (orb_gpu.hpp:40-42, orb_gpu.cpp:489-841), raw-plane form with an explicit row step (the reference assumes
    // step == width, orb_gpu.cpp:497).  The caller's SyncedMems are resized by the callee and receive the results on BOTH sides: the
    // device side by a device-to-device copy on the handle's stream, the host side from the handle's pinned mirror.
    void extract(const unsigned char *image, int step, SyncedMem<int> &out_keypoints, SyncedMem<unsigned char> &out_keypoints_desc)
    {
        // the caller's SyncedMems are sized once for the keypoint cap T (resize grows only), so that the handle can deliver the device
        // copies in the same stream round trip as the counts; count_ is then set to the frame's 6N / 32N
        const int T = jsorb_total_tiles(handle_);
        if (out_keypoints.capacity_ < 6 * T) out_keypoints.resize(6 * T);
        if (out_keypoints_desc.capacity_ < 32 * T) out_keypoints_desc.resize(32 * T);
        int n = 0;
        if (jsorb_extract_into(handle_, image, step, &n, out_keypoints.gpu_data_, out_keypoints_desc.gpu_data_) != JSORB_OK)
            throw std::runtime_error(std::string("jsorb_extract: ") + jsorb_last_error(handle_));
        out_keypoints.resize(6 * n);
        out_keypoints_desc.resize(32 * n);
        if (n > 0 && (jsorb_copy_keypoints(handle_, 0, out_keypoints.cpu_data_) != JSORB_OK ||             // host side: from the handle's pinned mirror
                      jsorb_copy_descriptors(handle_, 0, out_keypoints_desc.cpu_data_) != JSORB_OK))
            throw std::runtime_error("jsorb: delivering the extract results failed");
        out_keypoints.set_host_fresh(true); out_keypoints_desc.set_host_fresh(true);
    }
#ifdef JSORB_WITH_OPENCV
    void extract(const cv::Mat &image, SyncedMem<int> &out_keypoints, SyncedMem<unsigned char> &out_keypoints_desc)
    {
        extract(image.data, (int)image.step, out_keypoints, out_keypoints_desc);
    }
#endif

    // ORB_GPU::ORB_compute_stereo_match (orb_gpu.hpp:218-229, orb_stereo_match.cu:105-580) with the reference's parameter list, so
    // that Frame::ComputeStereoMatches (Frame.cpp:780-803) compiles unchanged.  It matches the LAST extract of the two handles - which
    // is what mvKeys / mvKeysRight / the descriptor pointers / the two pyramids describe at that call site; the keypoint vectors are
    // compared with the handles' own keypoints (below), the descriptor pointers are not read.  KeyPoint is cv::KeyPoint in the reference.
    template <class KeyPoint>
    void ORB_compute_stereo_match(int ORB_TH_HIGH, int ORB_TH_LOW, float mb, float mbf, std::vector<int> & /*octave_height*/, std::vector<int> & /*octave_width*/,
                                  std::vector<KeyPoint> &mvKeys, std::vector<KeyPoint> &mvKeysRight, std::vector<float> &mvuRight, std::vector<float> &mvDepth,
                                  unsigned char * /*descriptor_left_gpu*/, unsigned char * /*descriptor_right_gpu*/, ImagePyramid &images_left,
                                  ImagePyramid &images_right)
    {
        if (images_left.owner != this || !images_right.owner) throw std::invalid_argument("ORB_compute_stereo_match: pyramids do not belong to these extractors");
        jsorb_extractor *l = handle_, *r = images_right.owner->handle_;
        // Frame's stereo call shape (two extracts, then this call, every frame): ask the library to run the NEXT frame's match right behind
        // its two extracts on the GPU (jsorb.h, jsorb_set_speculative_stereo).  Opt-in here, not a library default: a mono / RGB-D
        // flow never reaches this function.
        if (!speculation_requested_) { jsorb_set_speculative_stereo(l, 1); speculation_requested_ = true; }
        const int n = jsorb_n_keypoints(l, 0);
        if (n < 0 || (size_t)n != mvKeys.size() || (size_t)jsorb_n_keypoints(r, 0) != mvKeysRight.size())
            throw std::runtime_error("ORB_compute_stereo_match: keypoint vectors do not match the last extract of the handles");
        // The reference READS mvKeys / mvKeysRight (orb_stereo_match.cu:119-184); this implementation matches what the handles extracted last.  A
        // caller that filtered, reordered or edited its keypoints in between would get silently different results, so the keypoint
        // vectors are compared with the handles' own (position and octave): all of them on the first call and in debug builds, a strided
        // sample afterwards.  JSORB_COMPAT_NO_KEYPOINT_CHECK removes the check (two device-to-host copies of 24 N bytes per call).
#ifndef JSORB_COMPAT_NO_KEYPOINT_CHECK
        {
#ifdef NDEBUG
            const size_t stride = keypoints_checked_ ? 16 : 1;
#else
            const size_t stride = 1;
#endif
            auto same = [&](jsorb_extractor *h, const std::vector<KeyPoint> &keys, std::vector<int32_t> &soa) {
                const size_t m = keys.size();
                if (!m) return true;
                soa.resize(6 * m);
                if (jsorb_copy_keypoints(h, 0, soa.data()) != JSORB_OK) return false;
                for (size_t i = 0; i < m; i += (i + stride < m || i + 1 == m) ? stride : m - 1 - i)      // the strided sample always includes the last one
                    if (keys[i].pt.x != (float)soa[i] || keys[i].pt.y != (float)soa[m + i] || keys[i].octave != soa[4 * m + i]) return false;
                return true;
            };
            if (!same(l, mvKeys, check_soa_) || !same(r, mvKeysRight, check_soa_))
                throw std::runtime_error("ORB_compute_stereo_match: mvKeys / mvKeysRight are not the keypoints of the handles' last extract (filtered or "
                                         "reordered?) - this implementation matches the last extract, see INTEGRATION.md");
            keypoints_checked_ = true;
        }
#endif
        mvuRight.resize(mvKeys.size(), -1.0f);          // orb_stereo_match.cu:496-497 (resize keeps earlier contents; the ABI call overwrites all n)
        mvDepth.resize(mvKeys.size(), -1.0f);
        float dummy = -1.0f;
        if (jsorb_stereo_match(l, r, mb, mbf, ORB_TH_HIGH, ORB_TH_LOW, n ? mvuRight.data() : &dummy, n ? mvDepth.data() : &dummy, &last_stereo_stats_) != JSORB_OK)
            throw std::runtime_error(std::string("jsorb_stereo_match: ") + jsorb_last_error(l));
    }

    jsorb_extractor *handle() const { return handle_; }

    // public data members of the reference that host code outside ORB_GPU reads (orb_gpu.hpp:240-250; Frame.cpp:784-801)
    int n_levels_ = 0;
    std::vector<int> height_, width_;
    std::vector<float> scale_, inv_scale_;
    ImagePyramid image_;
    jsorb_stereo_stats last_stereo_stats_{};
    bool speculation_requested_ = false;
    bool keypoints_checked_ = false;
    std::vector<int32_t> check_soa_;

private:
    jsorb_extractor *handle_ = nullptr;
};

} // namespace orb_cuda

namespace tracking_cuda {
// tracking_cuda::compute_isInFrustum_GPU (tracking_gpu.hpp:14-31, tracking_isinfrustum.cu:19-160): synchronous, device pointers
inline void compute_isInFrustum_GPU(int n_points, float *Px_gpu, float *Py_gpu, float *Pz_gpu, float *Pnx_gpu, float *Pny_gpu, float *Pnz_gpu,
                                    float *MaxDistance_gpu, float *invariance_maxDistance_gpu, float *invariance_minDistance_gpu, float *Rcw_gpu,
                                    float *tcw_gpu, float *Ow_gpu, float &fx, float &fy, float &cx, float &cy, int &minX, int &maxX, int &minY, int &maxY,
                                    int &nScaleLevels, float &logScaleFactor, float &viewCosAngle, float *invz_gpu, float *u_gpu, float *v_gpu,
                                    int *predictedlevel_gpu, float *viewCos_gpu, unsigned char *is_infrustum_gpu)
{
    if (jsorb_is_in_frustum(nullptr, n_points, Px_gpu, Py_gpu, Pz_gpu, Pnx_gpu, Pny_gpu, Pnz_gpu, MaxDistance_gpu, invariance_maxDistance_gpu,
                            invariance_minDistance_gpu, Rcw_gpu, tcw_gpu, Ow_gpu, fx, fy, cx, cy, minX, maxX, minY, maxY, nScaleLevels, logScaleFactor,
                            viewCosAngle, invz_gpu, u_gpu, v_gpu, predictedlevel_gpu, viewCos_gpu, is_infrustum_gpu) != JSORB_OK)
        throw std::runtime_error("jsorb_is_in_frustum failed");
}
} // namespace tracking_cuda

// The vocabulary tree on the device (jsorb_vocabulary, include/jsorb.h): RAII over the C calls.  Built from DBoW2's m_nodes flattened into host
// arrays (INTEGRATION.md shows the subclass of ORBVocabulary that does it); shared by every extractor on the device.
namespace jsorb {
class Vocabulary {
public:
    Vocabulary(int n_nodes, int depth_L, int levels_up, const int32_t *child_start, const int32_t *children, const unsigned char *descriptors,
               const int32_t *word_id, const double *weight, int device_id = 0)
    {
        const int rc = jsorb_vocabulary_create(device_id, n_nodes, depth_L, levels_up, child_start, children, descriptors, word_id, weight, &v_);
        if (rc != JSORB_OK) throw std::invalid_argument(rc == JSORB_ERR_INVALID ? "jsorb_vocabulary_create: the arrays are not a tree of this depth" : "jsorb_vocabulary_create failed");
    }
    Vocabulary(const Vocabulary &) = delete;
    Vocabulary &operator=(const Vocabulary &) = delete;
    ~Vocabulary() { jsorb_vocabulary_destroy(v_); }
    const jsorb_vocabulary *handle() const { return v_; }
    int words() const { int w = 0; jsorb_vocabulary_info(v_, nullptr, &w, nullptr, nullptr, nullptr); return w; }

private:
    jsorb_vocabulary *v_ = nullptr;
};
// A vocabulary trained on the device: what ORBVocabulary::create(training_features, k, L, weighting, scoring) leaves in m_nodes
// (jsorb_vocabulary_train, include/jsorb.h), as flat host arrays - node 0 the root, DBoW2's node ids and word ids - with Ni per node and the
// statistics of the run.
struct TrainedVocabulary {
    int n_nodes = 0, n_words = 0, k = 0, depth_L = 0, weighting = 0, scoring = 0;
    std::vector<int32_t> parent, child_start, children, word_id, Ni;
    std::vector<unsigned char> descriptors;      // n_nodes x 32
    std::vector<double> weight;
    int n_kmeans_runs = 0, n_empty_clusters = 0, n_unconverged = 0, lloyd_passes[16] = {0};
    long long n_draws = 0;
};
// vocabulary.create(training_features, k, L, weighting, scoring) for n descriptors on the DEVICE (n x 32 bytes, the documents concatenated;
// doc_start: the n_docs + 1 offsets of training_features[i]).  Waits for its work on hip_stream.
inline TrainedVocabulary TrainVocabulary(const unsigned char *descriptors_gpu, int n, const std::vector<int32_t> &doc_start, int k, int L, int weighting = 0,
                                         int scoring = 0, uint64_t seed = 0, int max_iterations = 0, void *hip_stream = nullptr, int device_id = 0)
{
    jsorb_vocab_train_result *r = nullptr;
    const int rc = jsorb_vocabulary_train(device_id, hip_stream, descriptors_gpu, n, doc_start.data(), (int)doc_start.size() - 1, k, L, weighting, scoring,
                                          seed, max_iterations, &r);
    if (rc == JSORB_ERR_INVALID) throw std::invalid_argument(jsorb_vocabulary_train_last_error());
    if (rc != JSORB_OK) throw std::runtime_error(jsorb_vocabulary_train_last_error());
    TrainedVocabulary t;
    jsorb_vocab_train_result_info(r, &t.n_nodes, &t.n_words, nullptr, &t.k, &t.depth_L, &t.weighting, &t.scoring);
    const size_t nn = (size_t)t.n_nodes;
    t.parent.resize(nn); t.child_start.resize(nn + 1); t.children.resize(nn - 1); t.word_id.resize(nn); t.Ni.resize(nn);
    t.descriptors.resize(nn * 32); t.weight.resize(nn);
    jsorb_vocab_train_result_copy(r, t.parent.data(), t.child_start.data(), t.children.data(), t.descriptors.data(), t.word_id.data(), t.weight.data(),
                                  t.Ni.data());
    jsorb_vocab_train_stats(r, &t.n_kmeans_runs, &t.n_draws, &t.n_empty_clusters, &t.n_unconverged, t.lloyd_passes);
    jsorb_vocab_train_result_destroy(r);
    return t;
}
// the device vocabulary of a trained tree (levels_up: the 4 of Frame::ComputeBoW)
inline std::unique_ptr<Vocabulary> MakeVocabulary(const TrainedVocabulary &t, int levels_up = 4, int device_id = 0)
{
    return std::unique_ptr<Vocabulary>(new Vocabulary(t.n_nodes, t.depth_L, levels_up, t.child_start.data(), t.children.data(), t.descriptors.data(),
                                                      t.word_id.data(), t.weight.data(), device_id));
}
// saveToTextFile (TemplatedVocabulary.h:1428-1457): `k L scoring weighting`, then per node `parent isLeaf b0 .. b31 weight` in node id order
// (the weight with 17 significant digits: it reads back to the same double)
inline bool SaveVocabularyText(const TrainedVocabulary &t, const std::string &path)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    fprintf(f, "%d %d %d %d\n", t.k, t.depth_L, t.scoring, t.weighting);
    for (int i = 1; i < t.n_nodes; i++) {
        fprintf(f, "%d %d ", t.parent[i], t.word_id[i] >= 0 ? 1 : 0);
        for (int b = 0; b < 32; b++) fprintf(f, "%d ", (int)t.descriptors[(size_t)i * 32 + b]);
        fprintf(f, "%.17g\n", t.weight[i]);
    }
    return fclose(f) == 0;
}
// The keyframe-to-keyframe matcher of LocalMapping (jsorb_keyframe_matcher, include/jsorb.h): RAII over the C calls.  It owns its stream and
// scratch, so LocalMapping's thread never touches Tracking's extractors.  One object per thread.
class KeyframeMatcher {
public:
    explicit KeyframeMatcher(int device_id = 0)
    {
        if (jsorb_keyframe_matcher_create(device_id, &m_) != JSORB_OK) throw std::runtime_error("jsorb_keyframe_matcher_create failed");
    }
    KeyframeMatcher(const KeyframeMatcher &) = delete;
    KeyframeMatcher &operator=(const KeyframeMatcher &) = delete;
    ~KeyframeMatcher() { jsorb_keyframe_matcher_destroy(m_); }
    jsorb_keyframe_matcher *handle() const { return m_; }
    void set_stream(void *hip_stream) { jsorb_keyframe_matcher_set_stream(m_, hip_stream); }
    void *stream() const { return jsorb_keyframe_matcher_get_stream(m_); }

private:
    jsorb_keyframe_matcher *m_ = nullptr;
};
// One side of SearchForTriangulation as DEVICE arrays (SyncedMem<T>::gpu_data() after to_gpu()): n keypoints; node = the FeatureVector node per
// keypoint (-1: none), is_free = GetMapPoint(i) == NULL, stereo = mvuRight[i] >= 0, x / y / angle / octave from mvKeysUn (octave: the KF2 side
// only), descriptors 32 bytes each.  The KF2 side holds all neighbours one after the other.
struct KeyframeSide {
    int n = 0;
    const int32_t *node = nullptr;
    const unsigned char *is_free = nullptr, *stereo = nullptr;
    const float *x = nullptr, *y = nullptr;
    const int32_t *octave = nullptr;
    const float *angle = nullptr;
    const unsigned char *descriptors = nullptr;
};
// The sides of Fuse as DEVICE arrays.  FusePoints: n map points - GetWorldPos, GetNormal, mfMaxDistance, GetMinDistanceInvariance,
// GetMaxDistanceInvariance and GetDescriptor (32 bytes each).  FuseKeyframes: the target keyframes one after the other - mvKeysUn as x / y /
// octave, mvuRight (nullptr: all monocular) and mDescriptors.  FusePoses: HOST arrays, per keyframe 9 floats of GetRotation (row-major), 3 of
// GetTranslation and 3 of GetCameraCenter.
struct FusePoints {
    int n = 0;
    const float *Px = nullptr, *Py = nullptr, *Pz = nullptr, *Nx = nullptr, *Ny = nullptr, *Nz = nullptr;
    const float *max_distance = nullptr, *min_dist_inv = nullptr, *max_dist_inv = nullptr;
    const unsigned char *descriptors = nullptr;
};
struct FuseKeyframes {
    const float *x = nullptr, *y = nullptr;
    const int32_t *octave = nullptr;
    const float *uright = nullptr;
    const unsigned char *descriptors = nullptr;
};
struct FusePoses {
    const float *Rcw = nullptr, *tcw = nullptr, *Ow = nullptr;
};
// One side of the loop-closing SearchByBoW(pKF1, pKF2, vpMatches12) as DEVICE arrays: n keypoints; node = the FeatureVector node per keypoint (-1:
// none), valid = pMP && !pMP->isBad() of GetMapPointMatches()[i], angle = mvKeysUn[i].angle, descriptors 32 bytes each.  The candidate side holds all
// loop candidates one after the other.
struct BowKeyframeSide {
    int n = 0;
    const int32_t *node = nullptr;
    const unsigned char *valid = nullptr;
    const float *angle = nullptr;
    const unsigned char *descriptors = nullptr;
};
// One side of SearchBySim3: jsorb_sim3_side (include/jsorb.h) with everything cleared - n slots aligned with the keyframe's keypoints as DEVICE
// arrays, and on the HOST the keyframe's own Rw / tw and the similarity sR / t into the other camera (side 1: sR21, t21; side 2: sR12, t12).
struct Sim3Side : jsorb_sim3_side {
    Sim3Side() : jsorb_sim3_side() {}
};
// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): a map point as that call reads it, HOST values - GetWorldPos, GetNormal, mfMaxDistance,
// GetMinDistanceInvariance, GetMaxDistanceInvariance, GetDescriptor and isBad() - and the keyframe's mvKeysUn (x / y / octave) and mDescriptors
// as DEVICE arrays, which a loop-closing thread keeps from SearchByBoW(KF, KF) and SearchBySim3.
struct ScwPoint {
    float pos[3] = {0, 0, 0}, normal[3] = {0, 0, 0};
    float max_distance = 0, min_dist_inv = 0, max_dist_inv = 0;
    unsigned char descriptor[32] = {};
    bool bad = false;
};
// The observations of n map points as DEVICE arrays, flat: obs_start[n + 1] the CSR, obs_row[n_obs] each observation's row of the concatenated
// keyframe descriptors kf_descriptors (n_rows x 32 bytes; the caller adds its kf_start[k] to the keypoint index) - per point in the order
// GetObservations() iterates, the keyframes that are isBad() left out.  out_row: nullptr (point p owns row p of the table) or n rows of it.
struct Observations {
    int n = 0, n_obs = 0, n_rows = 0;
    const int32_t *obs_start = nullptr, *obs_row = nullptr;
    const unsigned char *kf_descriptors = nullptr;
    const int32_t *out_row = nullptr;
};
struct ScwKeyframe {
    int n = 0;
    const float *x = nullptr, *y = nullptr;
    const int32_t *octave = nullptr;
    const unsigned char *descriptors = nullptr;
};
// A BowVector on the device (include/jsorb.h): `cap` entries of room in DEVICE arrays the caller owns, the count on the device.
struct DeviceBowVector {
    int32_t *word = nullptr;
    double *value = nullptr;
    int32_t *n = nullptr;
    int cap = 0;
};
// KeyFrameDatabase on the device (jsorb_keyframe_database, include/jsorb.h): RAII over the C calls.  A keyframe is a slot in [0, max_keyframes) the
// caller maps its KeyFrame* to; word_weight: the n_words leaf weights by word id, HOST.  It owns its stream and scratch.
class KeyframeDatabase {
public:
    KeyframeDatabase(int max_keyframes, int n_words, const double *word_weight, int device_id = 0) : max_keyframes_(max_keyframes)
    {
        if (jsorb_keyframe_database_create(device_id, max_keyframes, n_words, word_weight, &d_) != JSORB_OK)
            throw std::runtime_error("jsorb_keyframe_database_create failed");
    }
    KeyframeDatabase(const KeyframeDatabase &) = delete;
    KeyframeDatabase &operator=(const KeyframeDatabase &) = delete;
    ~KeyframeDatabase() { jsorb_keyframe_database_destroy(d_); }
    jsorb_keyframe_database *handle() const { return d_; }
    int max_keyframes() const { return max_keyframes_; }
    void set_stream(void *hip_stream) { jsorb_keyframe_database_set_stream(d_, hip_stream); }
    void *stream() const { return jsorb_keyframe_database_get_stream(d_); }
    // KeyFrameDatabase::add / erase / clear (KeyFrameDatabase.cpp:44-77)
    void add(int slot, const DeviceBowVector &v) { check(jsorb_keyframe_database_add_async(d_, slot, v.word, v.value, v.cap, v.n), "add"); }
    void erase(int slot) { check(jsorb_keyframe_database_erase(d_, slot), "erase"); }
    void clear() { check(jsorb_keyframe_database_clear(d_), "clear"); }
    void check(int rc, const char *what) const
    {
        if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb_keyframe_database ") + what + ": " + jsorb_keyframe_database_last_error(d_));
    }

private:
    jsorb_keyframe_database *d_ = nullptr;
    int max_keyframes_ = 0;
};
// What the device-state classes below share: the memory calls' error as an exception that names the class, and one owned device array.
namespace detail {
inline void check(int rc, const char *cls, const char *what)
{
    if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb::") + cls + " " + what + ": " + jsorb_mem_last_error());
}
// n elements of T on the device (at least one is allocated), all zero, all `fill` or left as they come (reserve); freed with the object, not
// copyable.  cls: the class that holds it, for the exceptions' texts.  put / get move one element and check its index against n; upload writes a
// span the caller has checked.
template <class T> class DeviceArray {
public:
    DeviceArray() = default;
    DeviceArray(const char *cls, size_t n) { alloc(cls, n); }
    DeviceArray(const char *cls, size_t n, T fill) { alloc(cls, n, fill); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    ~DeviceArray() { jsorb_mem_free_device(p_); }
    void reserve(const char *cls, size_t n)      // contents undefined (again: what it held before is freed)
    {
        jsorb_mem_free_device(p_);
        p_ = nullptr; cls_ = cls; n_ = n;
        check(jsorb_mem_alloc_device((n ? n : 1) * sizeof(T), (void **)&p_), cls_, "alloc");
    }
    void alloc(const char *cls, size_t n)
    {
        reserve(cls, n);
        check(jsorb_mem_set_zero(p_, (n ? n : 1) * sizeof(T)), cls_, "clear");
    }
    void alloc(const char *cls, size_t n, T fill)
    {
        reserve(cls, n);
        const std::vector<T> h(n ? n : 1, fill);
        upload(0, h.data(), h.size());
    }
    T *ptr() const { return p_; }      // NULL before alloc
    size_t size() const { return n_; }
    void upload(size_t at, const T *src, size_t n) { if (n) check(jsorb_mem_h2d(p_ + at, src, n * sizeof(T)), cls_, "upload"); }
    void put(long long i, T v) { check(jsorb_mem_h2d(p_ + in(i), &v, sizeof(T)), cls_, "upload"); }
    T get(long long i) const { T v = T(); check(jsorb_mem_d2h(&v, p_ + in(i), sizeof(T)), cls_, "copy back"); return v; }

private:
    size_t in(long long i) const
    {
        if (i < 0 || (size_t)i >= n_) throw std::runtime_error(std::string("jsorb::") + cls_ + ": index out of range");
        return (size_t)i;
    }
    T *p_ = nullptr;
    size_t n_ = 0;
    const char *cls_ = "";
};
} // namespace detail
// The map points as the device table jsorb_local_map_points reads (jsorb_map_point_table, include/jsorb.h): RAII over eleven device arrays of
// n_rows rows.  A row is the caller's index for a MapPoint* (INTEGRATION.md), the same as the rows of ComputeDistinctiveDescriptors' table, whose
// device array descriptors() is.  scatter() writes the rows a local BA, UpdateNormalAndDepth or SetBadFlag changed: one upload, one kernel.
class MapPointTable {
public:
    explicit MapPointTable(int n_rows) : n_rows_(n_rows), desc_(CLS, 32 * (size_t)(n_rows > 0 ? n_rows : 1)), bad_(CLS, n_rows > 0 ? n_rows : 0)
    {
        for (detail::DeviceArray<float> &f : f_) f.alloc(CLS, n_rows > 0 ? n_rows : 0);
    }
    int n_rows() const { return n_rows_; }
    unsigned char *descriptors() const { return desc_.ptr(); }      // n_rows x 32 bytes, DEVICE
    jsorb_map_point_table view() const
    {
        return jsorb_map_point_table{n_rows_, f_[0].ptr(), f_[1].ptr(), f_[2].ptr(), f_[3].ptr(), f_[4].ptr(), f_[5].ptr(), f_[6].ptr(), f_[7].ptr(), f_[8].ptr(),
                                     desc_.ptr(), bad_.ptr()};
    }
    // the changed rows and their records (host); hip_stream: the stream the table's readers run on (the extractor's)
    void scatter(const std::vector<int32_t> &rows, const std::vector<jsorb_map_point_record> &records, void *hip_stream = nullptr)
    {
        const size_t n = rows.size();
        if (records.size() != n) throw std::runtime_error("MapPointTable::scatter: one record per row");
        if (n == 0) return;
        if (n > rows_.size()) { rows_.reserve(CLS, n); rec_.reserve(CLS, n); }
        rows_.upload(0, rows.data(), n);
        rec_.upload(0, records.data(), n);
        detail::check(jsorb_map_points_scatter_async(hip_stream, n_rows_, f_[0].ptr(), f_[1].ptr(), f_[2].ptr(), f_[3].ptr(), f_[4].ptr(), f_[5].ptr(), f_[6].ptr(),
                                                     f_[7].ptr(), f_[8].ptr(), bad_.ptr(), (int)n, rows_.ptr(), rec_.ptr()),
                      CLS, "scatter");
        detail::check(jsorb_mem_stream_sync(hip_stream), CLS, "sync");      // (the staging arrays are reused by the next scatter)
    }
    // n descriptor rows from the host, from row `first` on (a map whose descriptors are not picked on the device)
    void set_descriptors(int first, int n, const unsigned char *d) { if (n > 0) desc_.upload(32 * (size_t)first, d, 32 * (size_t)n); }

private:
    static constexpr const char *CLS = "MapPointTable";
    int n_rows_ = 0;
    detail::DeviceArray<float> f_[9];
    detail::DeviceArray<unsigned char> desc_, bad_;
    detail::DeviceArray<int32_t> rows_;
    detail::DeviceArray<jsorb_map_point_record> rec_;
};
// What UpdateLocalPoints leaves on the device for SearchLocalPoints: `capacity` slots, the map points inside the frustum first, in the order of
// mvpLocalMapPoints; point_row[i] (host) is the table row of slot i, -1 behind the last; counts as jsorb_local_map_points defines them.
struct LocalMapPoints {
    orb_cuda::SyncedMem<float> u, v, invz, viewCos;
    orb_cuda::SyncedMem<int> predictedlevel, point_row_gpu;
    orb_cuda::SyncedMem<unsigned char> isinfrustum, descriptors, blocked;
    std::vector<int32_t> point_row;
    int32_t counts[5] = {0, 0, 0, 0, 0};
    int capacity = 0;
};
// What Optimizer::PoseOptimization reads of the frame besides its keypoints (jsorb_pose_params, include/jsorb.h): pFrame->fx, fy, cx, cy, mbf and
// mvInvLevelSigma2 (up to JSORB_MAX_LEVELS levels, the rest 0)
struct PoseParams : jsorb_pose_params {
    PoseParams(float fx_, float fy_, float cx_, float cy_, float mbf, const std::vector<float> &mvInvLevelSigma2)
    {
        if (mvInvLevelSigma2.size() > JSORB_MAX_LEVELS) throw std::runtime_error("jsorb::PoseParams: more than JSORB_MAX_LEVELS levels");
        fx = fx_; fy = fy_; cx = cx_; cy = cy_; bf = mbf;
        for (int l = 0; l < JSORB_MAX_LEVELS; l++) inv_level_sigma2[l] = (size_t)l < mvInvLevelSigma2.size() ? mvInvLevelSigma2[l] : 0.0f;
    }
};
// The keyframes as the device arrays jsorb_local_keyframes reads (jsorb_keyframe_graph, include/jsorb.h): RAII over eleven device arrays of
// max_keyframes slots, the caller's index for a KeyFrame* as for KeyframeDatabase.  The binding calls a setter where the reference changes the
// map (INTEGRATION.md lists which event rewrites which array); each setter is one small upload.  Runs are handed out from the pools front to
// back and rewritten in place while they fit; a full pool throws.
class KeyframeGraph {
    using Ints = detail::DeviceArray<int32_t>;
    using Bytes = detail::DeviceArray<unsigned char>;

public:
    enum { ABSENT = 0, GOOD = 1, BAD = 2 };
    KeyframeGraph(int max_keyframes, int pool_entries, int child_entries)
        : S_(max_keyframes), pool_(pool_entries), child_(child_entries), state_(CLS, slots()), registered_(CLS, entries(pool_), 1), key_(CLS, slots()),
          point_off_(CLS, slots()), point_len_(CLS, slots()), point_pool_(CLS, entries(pool_), -1), neighbours_(CLS, 10 * slots(), -1), child_off_(CLS, slots()),
          child_len_(CLS, slots()), child_pool_(CLS, entries(child_), -1), parent_(CLS, slots(), -1)
    {
        point_run_.assign(slots(), {0, -1}); child_run_.assign(slots(), {0, -1}); point_n_.assign(slots(), 0);
    }
    int max_keyframes() const { return S_; }
    int pool_entries() const { return pool_; }
    int point_offset(int slot) const { return point_run_[in(slot)].first; }        // where the slot's run starts in point_pool (set_keyframe)
    int point_length(int slot) const { return point_n_[in(slot)]; }                // the entries of the slot's run (set_keyframe; 0 after erase)
    jsorb_keyframe_graph view() const
    {
        return jsorb_keyframe_graph{S_, pool_, child_, state_.ptr(), key_.ptr(), point_off_.ptr(), point_len_.ptr(), point_pool_.ptr(), registered_.ptr(),
                                    neighbours_.ptr(), child_off_.ptr(), child_len_.ptr(), child_pool_.ptr(), parent_.ptr()};
    }
    // GetMapPointMatches() as table rows (-1 = NULL), (intptr_t)pKF, the state, and per entry whether the point holds the keyframe in mObservations
    void set_keyframe(int slot, const std::vector<int32_t> &rows, int64_t key, int state = GOOD, const std::vector<unsigned char> *registered = nullptr)
    {
        const int at = write_run(slot, rows, point_run_, point_used_, pool_, point_pool_, point_off_, point_len_);
        point_n_[slot] = (int)rows.size();
        if (!rows.empty()) {
            std::vector<unsigned char> ones;
            if (!registered) { ones.assign(rows.size(), 1); registered = &ones; }
            if (registered->size() != rows.size()) throw std::runtime_error("KeyframeGraph::set_keyframe: one registered byte per row");
            registered_.upload(at, registered->data(), rows.size());
        }
        key_.put(slot, key);
        set_state(slot, state);
    }
    void set_state(int slot, int state) { state_.put(in(slot), (unsigned char)state); }
    void set_neighbours(int slot, const std::vector<int32_t> &slots)      // GetBestCovisibilityKeyFrames(10), in its order
    {
        int32_t row[10];
        for (int i = 0; i < 10; i++) row[i] = i < (int)slots.size() ? slots[i] : -1;
        neighbours_.upload(10 * (size_t)in(slot), row, 10);
    }
    void set_children(int slot, const std::vector<int32_t> &slots) { write_run(slot, slots, child_run_, child_used_, child_, child_pool_, child_off_, child_len_); }      // GetChilds(), std::set's order
    void set_parent(int slot, int parent) { parent_.put(in(slot), parent); }
    void erase(int slot)
    {
        set_state(slot, ABSENT); point_len_.put(slot, 0); child_len_.put(slot, 0); set_parent(slot, -1); set_neighbours(slot, {});
        point_n_[slot] = 0;
    }

private:
    static constexpr const char *CLS = "KeyframeGraph";
    size_t slots() const { return S_ > 0 ? S_ : 1; }      // (the host vectors and the per-slot arrays have at least one entry)
    static size_t entries(int n) { return n > 0 ? n : 1; }
    int in(int slot) const      // (it also guards the host vectors, so it stays the class's own)
    {
        if (slot < 0 || slot >= S_) throw std::runtime_error("jsorb::KeyframeGraph: slot outside [0, max_keyframes)");
        return slot;
    }
    int write_run(int slot, const std::vector<int32_t> &v, std::vector<std::pair<int, int>> &runs, int &used, int total, Ints &pool, Ints &off, Ints &len)
    {
        std::pair<int, int> &r = runs[in(slot)];       // (offset, entries reserved)
        const int n = (int)v.size();
        if (n > r.second) {
            if (used + n > total) throw std::runtime_error("jsorb::KeyframeGraph: pool full");
            r = {used, n};
            used += n;
        }
        pool.upload(r.first, v.data(), n);
        off.put(slot, r.first); len.put(slot, n);
        return r.first;
    }
    int S_ = 0, pool_ = 0, child_ = 0, point_used_ = 0, child_used_ = 0;
    Bytes state_, registered_;
    detail::DeviceArray<int64_t> key_;
    Ints point_off_, point_len_, point_pool_, neighbours_, child_off_, child_len_, child_pool_, parent_;
    std::vector<std::pair<int, int>> point_run_, child_run_;
    std::vector<int> point_n_;
};
// mvpLocalKeyFrames and mpReferenceKF as UpdateLocalKeyFrames keeps them from frame to frame, and the local keyframes' rows concatenated for
// UpdateLocalPoints: slots[i] (host) the slot of the i-th local keyframe, ref_slot the slot of mpReferenceKF (-1: none yet), counts as
// jsorb_local_keyframes defines them; the device arrays hold the persistent state the next call reads.
struct LocalKeyFrames {
    LocalKeyFrames(int kf_capacity_, int entry_capacity_) : kf_capacity(kf_capacity_), entry_capacity(entry_capacity_)
    {
        slot_gpu.resize(kf_capacity); start_gpu.resize(kf_capacity + 1); point_row_gpu.resize(entry_capacity > 0 ? entry_capacity : 1);
        state_gpu.resize(2); counts_gpu.resize(8);
        slot_gpu.set_zero_gpu();
        state_gpu.cpu_data()[0] = 0; state_gpu.cpu_data()[1] = -1;
        state_gpu.to_gpu();
    }
    orb_cuda::SyncedMem<int> slot_gpu, state_gpu, start_gpu, point_row_gpu, counts_gpu;
    std::vector<int32_t> slots;
    int ref_slot = -1;
    int32_t counts[8] = {0, 0, 0, -1, 0, 0, 0, 0};
    int kf_capacity, entry_capacity;
};
// The covisibility graph as jsorb_update_connections keeps it on the device (jsorb_covisibility, include/jsorb.h): RAII over seven device arrays
// of max_keyframes slots, conn_capacity entries per slot, all zero at first.  created(slot) is the binding's part of the KeyFrame constructor.
class Covisibility {
public:
    Covisibility(int max_keyframes, int conn_capacity) : S_(max_keyframes), C_(conn_capacity)
    {
        int lo = 0, hi = 0;
        jsorb_covisibility_build_caps(&lo, &hi);
        if (C_ < lo || C_ > hi) throw std::runtime_error("jsorb::Covisibility: conn_capacity outside the library's bounds");
        const size_t s = S_ > 0 ? S_ : 0, row = s ? s * C_ : (size_t)C_;      // (an empty graph still has one slot's arrays)
        conn_len_.alloc(CLS, s); ord_len_.alloc(CLS, s); first_.alloc(CLS, s);
        conn_slot_.alloc(CLS, row); conn_weight_.alloc(CLS, row); ord_slot_.alloc(CLS, row); ord_weight_.alloc(CLS, row);
        v_ = jsorb_covisibility{S_, C_, conn_len_.ptr(), conn_slot_.ptr(), conn_weight_.ptr(), ord_len_.ptr(), ord_slot_.ptr(), ord_weight_.ptr(), first_.ptr()};
    }
    int max_keyframes() const { return S_; }
    int conn_capacity() const { return C_; }
    const jsorb_covisibility &view() const { return v_; }
    // a new keyframe in `slot`: empty map and lists; mbFirstConnection && mnId != 0
    void created(int slot, bool first_keyframe = false)
    {
        if (slot < 0 || slot >= S_) throw std::runtime_error("jsorb::Covisibility: slot outside [0, max_keyframes)");
        conn_len_.put(slot, 0); ord_len_.put(slot, 0); first_.put(slot, first_keyframe ? 0 : 1);
    }
    // one slot on the host (it waits for the device): the map in (order_key, slot) order and the ordered lists
    struct Slot {
        std::vector<int32_t> conn_slot, conn_weight, ord_slot, ord_weight;
    };
    Slot copy(int slot) const
    {
        Slot o;
        int32_t lens[2] = {0, 0};
        o.conn_slot.resize(C_); o.conn_weight.resize(C_); o.ord_slot.resize(C_); o.ord_weight.resize(C_);
        if (jsorb_covisibility_copy(&v_, slot, lens, o.conn_slot.data(), o.conn_weight.data(), o.ord_slot.data(), o.ord_weight.data()) != JSORB_OK)
            throw std::runtime_error("jsorb_covisibility_copy failed");
        const int nc = lens[0] < 0 ? 0 : lens[0] > C_ ? C_ : lens[0], no = lens[1] < 0 ? 0 : lens[1] > C_ ? C_ : lens[1];
        o.conn_slot.resize(nc); o.conn_weight.resize(nc); o.ord_slot.resize(no); o.ord_weight.resize(no);
        return o;
    }

private:
    static constexpr const char *CLS = "Covisibility";
    int S_ = 0, C_ = 0;
    detail::DeviceArray<int32_t> conn_len_, conn_slot_, conn_weight_, ord_len_, ord_slot_, ord_weight_;
    detail::DeviceArray<unsigned char> first_;
    jsorb_covisibility v_{};
};
// What KeyFrameCulling reads of the keyframes' keypoints (jsorb_keyframe_views, include/jsorb.h): device arrays parallel to the graph's
// point_pool - mvKeysUn[i].octave, mvuRight[i] >= 0, mvDepth[i] (none for a monocular map) - and mThDepth per slot.
class KeyframeViews {
public:
    KeyframeViews(const KeyframeGraph &graph, bool with_depth)
        : pool_(graph.pool_entries()), octave_(CLS, entries()), stereo_(CLS, entries()), th_depth_(CLS, graph.max_keyframes() > 0 ? graph.max_keyframes() : 0)
    {
        if (with_depth) depth_.alloc(CLS, entries());
    }
    jsorb_keyframe_views view() const { return jsorb_keyframe_views{pool_, octave_.ptr(), stereo_.ptr(), depth_.ptr(), th_depth_.ptr()}; }
    // the keyframe in `slot`, one entry per entry of its run (after graph.set_keyframe); depth may be NULL for a monocular map
    void set_keyframe_views(const KeyframeGraph &graph, int slot, const std::vector<unsigned char> &octave, const std::vector<unsigned char> &stereo,
                            const std::vector<float> *depth, float th_depth)
    {
        const size_t at = (size_t)graph.point_offset(slot), n = octave.size();
        if (stereo.size() != n || (depth && depth->size() != n) || at + n > entries() || (depth_.ptr() && !depth))
            throw std::runtime_error("jsorb::KeyframeViews: one octave, stereo and depth entry per entry of the run");
        octave_.upload(at, octave.data(), n);
        stereo_.upload(at, stereo.data(), n);
        if (depth_.ptr()) depth_.upload(at, depth->data(), n);
        th_depth_.put(slot, th_depth);
    }

private:
    static constexpr const char *CLS = "KeyframeViews";
    size_t entries() const { return pool_ > 0 ? pool_ : 0; }
    int pool_ = 0;
    detail::DeviceArray<unsigned char> octave_, stereo_;
    detail::DeviceArray<float> depth_, th_depth_;
};
// The arrays jsorb_cull_keyframes writes (jsorb_culling_state): the graph's and the table's own arrays once more as writable pointers, and
// mbNotErase / mbToBeErased per slot and the slot of mpRefKF per table row, which this class owns (zeros, zeros, -1).
class CullingState {
public:
    CullingState(const KeyframeGraph &graph, const MapPointTable &table)
        : not_erase_(CLS, count(graph.max_keyframes())), to_be_erased_(CLS, count(graph.max_keyframes())), ref_slot_(CLS, count(table.n_rows()), -1)
    {
        const jsorb_keyframe_graph g = graph.view();
        const jsorb_map_point_table t = table.view();
        v_ = jsorb_culling_state{const_cast<uint8_t *>(g.state), const_cast<uint8_t *>(g.registered), const_cast<uint8_t *>(t.bad),
                                 const_cast<int32_t *>(g.point_pool), const_cast<int32_t *>(g.parent), not_erase_.ptr(), to_be_erased_.ptr(), ref_slot_.ptr()};
    }
    const jsorb_culling_state &view() const { return v_; }
    void set_not_erase(int slot, bool on) { not_erase_.put(slot, on); }       // SetNotErase / SetErase
    void set_ref_slot(int row, int slot) { ref_slot_.put(row, slot); }        // mpRefKF
    bool to_be_erased(int slot) const { return to_be_erased_.get(slot) != 0; }
    int ref_slot(int row) const { return ref_slot_.get(row); }

private:
    static constexpr const char *CLS = "CullingState";
    static size_t count(int n) { return n > 0 ? n : 0; }
    detail::DeviceArray<unsigned char> not_erase_, to_be_erased_;
    detail::DeviceArray<int32_t> ref_slot_;
    jsorb_culling_state v_{};
};
// What ORBmatcher::Fuse reads of the keyframes' keypoints (jsorb_keyframe_keypoints, include/jsorb.h): device arrays parallel to the graph's
// point_pool - mvKeysUn (x, y, octave), mvuRight (none for a monocular map) and the descriptors.
class KeyframeKeypoints {
public:
    KeyframeKeypoints(const KeyframeGraph &graph, bool stereo)
        : pool_(graph.pool_entries()), x_(CLS, entries()), y_(CLS, entries()), octave_(CLS, entries()), desc_(CLS, 32 * (entries() ? entries() : 1))
    {
        if (stereo) uright_.alloc(CLS, entries(), -1.0f);
    }
    jsorb_keyframe_keypoints view() const { return jsorb_keyframe_keypoints{pool_, x_.ptr(), y_.ptr(), octave_.ptr(), uright_.ptr(), desc_.ptr()}; }
    // the keyframe in `slot`, one entry per entry of its run (after graph.set_keyframe); uright may be NULL (a monocular keyframe); desc: 32 bytes each
    void set_keyframe(const KeyframeGraph &graph, int slot, const std::vector<float> &x, const std::vector<float> &y, const std::vector<int32_t> &octave,
                      const std::vector<float> *uright, const std::vector<unsigned char> &desc)
    {
        const size_t at = (size_t)graph.point_offset(slot), n = x.size();
        if (n != (size_t)graph.point_length(slot) || y.size() != n || octave.size() != n || desc.size() != 32 * n || (uright && uright->size() != n) ||
            at + n > entries() || (uright && !uright_.ptr()))
            throw std::runtime_error("jsorb::KeyframeKeypoints: one x, y, octave, uright and descriptor per entry of the run");
        x_.upload(at, x.data(), n);
        y_.upload(at, y.data(), n);
        octave_.upload(at, octave.data(), n);
        desc_.upload(32 * at, desc.data(), 32 * n);
        if (uright_.ptr()) {
            const std::vector<float> none(n, -1.0f);
            uright_.upload(at, uright ? uright->data() : none.data(), n);
        }
    }

private:
    static constexpr const char *CLS = "KeyframeKeypoints";
    size_t entries() const { return pool_ > 0 ? pool_ : 0; }
    int pool_ = 0;
    detail::DeviceArray<float> x_, y_, uright_;
    detail::DeviceArray<int32_t> octave_;
    detail::DeviceArray<unsigned char> desc_;
};
// The arrays jsorb_fuse_map writes (jsorb_fuse_state): the graph's point_pool / registered and the table's bad / desc once more as writable
// pointers, and mpReplaced as a row (-1), mnVisible and mnFound per table row, which this class owns.
class FuseState {
public:
    FuseState(const KeyframeGraph &graph, const MapPointTable &table)
        : replaced_(CLS, rows(table), -1), visible_(CLS, rows(table)), found_(CLS, rows(table))
    {
        const jsorb_keyframe_graph g = graph.view();
        const jsorb_map_point_table t = table.view();
        v_ = jsorb_fuse_state{const_cast<int32_t *>(g.point_pool), const_cast<uint8_t *>(g.registered), const_cast<uint8_t *>(t.bad), const_cast<uint8_t *>(t.desc),
                              replaced_.ptr(), visible_.ptr(), found_.ptr()};
    }
    const jsorb_fuse_state &view() const { return v_; }
    int replaced(int row) const { return replaced_.get(row); }      // mpReplaced as a row, -1
    int visible(int row) const { return visible_.get(row); }
    int found(int row) const { return found_.get(row); }
    void set_counters(int row, int visible, int found) { visible_.put(row, visible); found_.put(row, found); }      // mnVisible, mnFound

private:
    static constexpr const char *CLS = "FuseState";
    static size_t rows(const MapPointTable &table) { return table.n_rows() > 0 ? table.n_rows() : 0; }
    detail::DeviceArray<int32_t> replaced_, visible_, found_;
    jsorb_fuse_state v_{};
};
// What CreateNewMapPoints reads of the keyframes' keypoints beyond KeyframeKeypoints (jsorb_new_point_keypoints, include/jsorb.h): device arrays
// parallel to the graph's point_pool - the mFeatVec node of every keypoint (-1: none), and for a stereo map mvDepth, cos(2*atan2(mb/2, mvDepth[i]))
// from the host's libm, and mvKeys (which KeyFrame::UnprojectStereo reads).
class NewPointKeypoints {
public:
    NewPointKeypoints(const KeyframeGraph &graph, bool stereo) : pool_(graph.pool_entries()), node_(CLS, entries(), -1)
    {
        if (stereo) { depth_.alloc(CLS, entries(), -1.0f); cos_.alloc(CLS, entries(), 1.0f); raw_x_.alloc(CLS, entries()); raw_y_.alloc(CLS, entries()); }
    }
    jsorb_new_point_keypoints view() const { return jsorb_new_point_keypoints{node_.ptr(), depth_.ptr(), raw_x_.ptr(), raw_y_.ptr(), cos_.ptr()}; }
    // the keyframe in `slot`, one entry per entry of its run (after graph.set_keyframe); the last four may be NULL for a monocular keyframe
    void set_keyframe(const KeyframeGraph &graph, int slot, const std::vector<int32_t> &node, const std::vector<float> *depth, const std::vector<float> *cos_stereo,
                      const std::vector<float> *raw_x, const std::vector<float> *raw_y)
    {
        const size_t at = (size_t)graph.point_offset(slot), n = node.size();
        const std::vector<float> *const f[4] = {depth, cos_stereo, raw_x, raw_y};
        bool ok = n == (size_t)graph.point_length(slot) && at + n <= entries();
        for (const std::vector<float> *v : f) ok = ok && (!v || (v->size() == n && depth_.ptr()));
        if (!ok) throw std::runtime_error("jsorb::NewPointKeypoints: one node, depth, cos_stereo and raw point per entry of the run");
        node_.upload(at, node.data(), n);
        detail::DeviceArray<float> *const d[4] = {&depth_, &cos_, &raw_x_, &raw_y_};
        for (int i = 0; i < 4; i++)
            if (f[i]) d[i]->upload(at, f[i]->data(), n);
    }

private:
    static constexpr const char *CLS = "NewPointKeypoints";
    size_t entries() const { return pool_ > 0 ? pool_ : 0; }
    int pool_ = 0;
    detail::DeviceArray<int32_t> node_;
    detail::DeviceArray<float> depth_, cos_, raw_x_, raw_y_;
};
// The arrays jsorb_create_new_map_points writes (jsorb_new_point_state): the graph's point_pool / registered and the table's arrays once more as
// writable pointers, and mpRefKF as a slot, mpReplaced as a row, mnVisible, mnFound and mnFirstKFid per table row, which this class owns.
class NewPointState {
public:
    NewPointState(const KeyframeGraph &graph, const MapPointTable &table)
        : ref_slot_(CLS, rows(table), -1), replaced_(CLS, rows(table), -1), visible_(CLS, rows(table)), found_(CLS, rows(table)), first_kf_id_(CLS, rows(table), -1)
    {
        const jsorb_keyframe_graph g = graph.view();
        const jsorb_map_point_table t = table.view();
        auto w = [](const float *p) { return const_cast<float *>(p); };
        v_ = jsorb_new_point_state{const_cast<int32_t *>(g.point_pool), const_cast<uint8_t *>(g.registered), const_cast<uint8_t *>(t.bad),
                                   const_cast<uint8_t *>(t.desc), w(t.Px), w(t.Py), w(t.Pz), w(t.Pnx), w(t.Pny), w(t.Pnz), w(t.MaxDistance),
                                   w(t.invariance_maxDistance), w(t.invariance_minDistance), ref_slot_.ptr(), replaced_.ptr(), visible_.ptr(), found_.ptr(),
                                   first_kf_id_.ptr()};
    }
    const jsorb_new_point_state &view() const { return v_; }
    int ref_slot(int row) const { return ref_slot_.get(row); }            // mpRefKF as a slot
    int first_kf_id(int row) const { return first_kf_id_.get(row); }      // mnFirstKFid

private:
    static constexpr const char *CLS = "NewPointState";
    static size_t rows(const MapPointTable &table) { return table.n_rows() > 0 ? table.n_rows() : 0; }
    detail::DeviceArray<int32_t> ref_slot_, replaced_, visible_, found_, first_kf_id_;
    jsorb_new_point_state v_{};
};
// What CreateNewMapPoints gives back: per (neighbour, idx1) the verdict (jsorb.h: 0 no match, 1 created, 2 taken, 3 .. 10 the gates, 11 no row, 12
// empty unprojection, 13 skipped neighbour), the path (1 SVD, 2 / 3 UnprojectStereo) and x3D; the new points in creation order as (row, idx1,
// neighbour, idx2) - what `new MapPoint`, the two AddObservation and the two AddMapPoint of the host objects follow; the counts.
struct NewMapPoints {
    std::vector<int32_t> verdict;
    std::vector<unsigned char> path;
    std::vector<float> x3D;
    std::vector<std::array<int32_t, 4>> created;
    int32_t counts[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
// What FuseMap gives back: per (target, list point) the keypoint searched (-1: none) with its distance and, for the overload with Scw,
// vpReplacePoint as a row; nFused per target; the Replace (2, p, q, -1) and AddMapPoint (3, row, slot, keypoint) events in order; the counts of
// jsorb_fuse_map.
struct FusedMap {
    std::vector<int32_t> best_idx, best_dist, replace_point, n_fused;
    std::vector<std::array<int32_t, 4>> events;
    int32_t counts[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
// What KeyFrameCulling gives back: per candidate of the current keyframe's list the decision (0 kept, 1 culled, 2 deferred by mbNotErase,
// 3 skipped) with n_mps and n_redundant as seen at its turn, the culled slots in order, every ChangeParent as (child, new parent) in order, and
// the counts of jsorb_cull_keyframes summed over the calls (counts[0] = the candidates).
struct CulledKeyFrames {
    std::vector<int32_t> candidates, decision, n_mps, n_redundant, culled;
    std::vector<std::pair<int32_t, int32_t>> reparent;
    int32_t counts[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
// a few device words for the length of a call
struct DeviceInts {
    explicit DeviceInts(size_t n) { words.reserve("DeviceInts", n); p = words.ptr(); }
    detail::DeviceArray<int32_t> words;
    int32_t *p = nullptr;
};
// What UpdateConnections gives back for its keyframes: parent[i] = the slot the binding makes mpParent of slots[i] (AddChild on it), -1 = none;
// counts as jsorb_update_connections defines them.
struct UpdatedConnections {
    std::vector<int32_t> parent;
    int32_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
} // namespace jsorb

namespace Jetson_SLAM {

using orb_cuda::SyncedMem;

class ORBExtractor {
public:
    // argument order of include/ORBextractor.h:25-35; str_mask: "" = no mask, else an image file (see ORB_GPU above)
    ORBExtractor(int im_height, int im_width, float scale_factor, int n_levels, int FAST_N_MIN, int FAST_N_MAX, int th_FAST_MIN,
                 int th_FAST_MAX, std::string str_mask, int tile_h, int tile_w, bool fixed_multi_scale_tile_size, bool apply_nms_ms,
                 bool nms_ms_mode_gpu, bool use_gpu = false)
    {
        init(im_height, im_width, scale_factor, n_levels, use_gpu);
        // src/ORBextractor.cpp:75-87 (the GPU object is built whatever use_gpu says; device 0)
        orb_gpu_ = new orb_cuda::ORB_GPU(im_height, im_width, n_levels, scale_factor, FAST_N_MIN, FAST_N_MAX, th_FAST_MIN, th_FAST_MAX, tile_h, tile_w,
                                         fixed_multi_scale_tile_size, apply_nms_ms, nms_ms_mode_gpu, str_mask, 0);
    }
    // additions: the mask as a decoded level-0 plane (NULL = none), an explicit device, a batch capacity
    ORBExtractor(int im_height, int im_width, float scale_factor, int n_levels, int FAST_N_MIN, int FAST_N_MAX, int th_FAST_MIN,
                 int th_FAST_MAX, const unsigned char *mask_plane, int tile_h, int tile_w, bool fixed_multi_scale_tile_size,
                 bool apply_nms_ms, bool nms_ms_mode_gpu, bool use_gpu = false, int device_id = 0, int max_batch = 1)
    {
        init(im_height, im_width, scale_factor, n_levels, use_gpu);
        orb_gpu_ = new orb_cuda::ORB_GPU(im_height, im_width, n_levels, scale_factor, FAST_N_MIN, FAST_N_MAX, th_FAST_MIN, th_FAST_MAX, tile_h, tile_w,
                                         fixed_multi_scale_tile_size, apply_nms_ms, nms_ms_mode_gpu, std::string(), device_id, mask_plane, max_batch);
    }
    ORBExtractor(const ORBExtractor &) = delete;
    ORBExtractor &operator=(const ORBExtractor &) = delete;
    ~ORBExtractor() { delete orb_gpu_; }

    // raw-plane form of extract(const cv::Mat&, SyncedMem<int>&, SyncedMem<unsigned char>&)  (ORBextractor.h:40-42)
    void extract(const unsigned char *image, int step, SyncedMem<int> &keypoints, SyncedMem<unsigned char> &keypoints_desc)
    {
        orb_gpu_->extract(image, step, keypoints, keypoints_desc);
    }
#ifdef JSORB_WITH_OPENCV
    void extract(const cv::Mat &image, SyncedMem<int> &keypoints, SyncedMem<unsigned char> &keypoints_desc) { orb_gpu_->extract(image, keypoints, keypoints_desc); }
    void operator()(const cv::Mat &image, SyncedMem<int> &k, SyncedMem<unsigned char> &d) { extract(image, k, d); }
#endif

    int get_levels() { return n_levels_; }
    float get_scale_factor() { return scale_factor_; }
    const std::vector<float> get_scale_factors() { return scale_; }
    std::vector<float> get_inverse_scale_factors() { return inv_scale_; }
    std::vector<float> get_scale_sigma_squares() { return level_sigma2_; }
    std::vector<float> get_inverse_scale_sigma_squares() { return inv_level_sigma2_; }

    orb_cuda::ORB_GPU *orb_gpu_ = nullptr;   // ORBextractor.h:75
    jsorb_extractor *handle() const { return orb_gpu_->handle(); }

protected:
    void init(int im_height, int im_width, float scale_factor, int n_levels, bool use_gpu)
    {
        n_levels_ = n_levels;
        scale_factor_ = scale_factor;
        use_gpu_ = use_gpu;
        // src/ORBextractor.cpp:43-71
        scale_.resize(n_levels); inv_scale_.resize(n_levels); level_sigma2_.resize(n_levels); inv_level_sigma2_.resize(n_levels);
        scale_[0] = 1.0f; level_sigma2_[0] = 1.0f;
        for (int i = 1; i < n_levels; i++) { scale_[i] = scale_[i - 1] * scale_factor_; level_sigma2_[i] = scale_[i] * scale_[i]; }
        for (int i = 0; i < n_levels; i++) { inv_scale_[i] = 1.0f / scale_[i]; inv_level_sigma2_[i] = 1.0f / level_sigma2_[i]; }
        width_.assign(1, im_width); height_.assign(1, im_height);
    }
    std::vector<int> height_, width_;
    std::vector<float> scale_, inv_scale_, level_sigma2_, inv_level_sigma2_;
    int n_levels_ = 0;
    float scale_factor_ = 1.f;
    bool use_gpu_ = false;
};

// Free-function form of Frame::ComputeStereoMatches (Frame.cpp:780-803): mvuRight / mvDepth sized N_left, -1 = no match.
// TH_HIGH / TH_LOW are ORBmatcher's (ORBmatcher.cpp:24-25).  mb must be mbf/fx (the reference reads an unassigned Frame::mb here on a
// fresh Frame, Frame.cpp:219 vs :247).
inline void ComputeStereoMatches(ORBExtractor &left, ORBExtractor &right, float mb, float mbf, std::vector<float> &mvuRight,
                                 std::vector<float> &mvDepth, jsorb_stereo_stats *stats = nullptr, int TH_HIGH = 100, int TH_LOW = 50)
{
    const int n = jsorb_n_keypoints(left.handle(), 0);
    if (n < 0) throw std::runtime_error("ComputeStereoMatches before extract");
    if (!left.orb_gpu_->speculation_requested_) { jsorb_set_speculative_stereo(left.handle(), 1); left.orb_gpu_->speculation_requested_ = true; }
    mvuRight.assign(n, -1.0f);
    mvDepth.assign(n, -1.0f);
    float dummy = -1.0f;
    const int rc = jsorb_stereo_match(left.handle(), right.handle(), mb, mbf, TH_HIGH, TH_LOW, n ? mvuRight.data() : &dummy, n ? mvDepth.data() : &dummy, stats);
    if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb_stereo_match: ") + jsorb_last_error(left.handle()));
}

// Body of the keypoint / descriptor unpacking of Frame::Frame (Frame.cpp:119-196) for one image: mvKeys-shaped records (the
// memory layout of cv::KeyPoint) and the N x 32 descriptor rows.
inline void UnpackFrame(ORBExtractor &ex, std::vector<jsorb_keypoint> &keys, std::vector<unsigned char> &descriptors)
{
    const int n = jsorb_n_keypoints(ex.handle(), 0);
    if (n < 0) throw std::runtime_error("UnpackFrame before extract");
    keys.resize(n);
    descriptors.resize((size_t)32 * n);
    if (n && jsorb_unpack_frame(ex.handle(), 0, keys.data(), descriptors.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_unpack_frame: ") + jsorb_last_error(ex.handle()));
}
#ifdef JSORB_WITH_OPENCV
inline void UnpackFrame(ORBExtractor &ex, std::vector<cv::KeyPoint> &mvKeys, cv::Mat &mDescriptors)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(jsorb_keypoint), "jsorb_keypoint mirrors cv::KeyPoint");
    const int n = jsorb_n_keypoints(ex.handle(), 0);
    if (n < 0) throw std::runtime_error("UnpackFrame before extract");
    mvKeys.resize(n);
    mDescriptors = cv::Mat(n, 32, CV_8UC1);
    if (n && jsorb_unpack_frame(ex.handle(), 0, reinterpret_cast<jsorb_keypoint *>(mvKeys.data()), mDescriptors.data) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_unpack_frame: ") + jsorb_last_error(ex.handle()));
}
#endif

// Body of Frame::AssignFeaturesToGrid (Frame.cpp:463-479) over mvKeysUn: the undistorted keypoints when the extractor has an active camera
// (SetCamera below: mono / RGB-D with lens distortion), the extracted ones otherwise (mvKeysUn == mvKeys: rectified stereo, k1 == 0).
// mGrid is the reference's std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS] (Frame.h:191).
template <std::size_t COLS, std::size_t ROWS>
inline void AssignFeaturesToGrid(ORBExtractor &ex, float mnMinX, float mnMinY, float mfGridElementWidthInv, float mfGridElementHeightInv,
                                 std::vector<std::size_t> (&mGrid)[COLS][ROWS])
{
    const int n = jsorb_n_keypoints(ex.handle(), 0);
    if (n < 0) throw std::runtime_error("AssignFeaturesToGrid before extract");
    std::vector<int32_t> start(COLS * ROWS + 1), items(n > 0 ? n : 1);
    if (jsorb_assign_features_to_grid(ex.handle(), 0, mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv, (int)COLS, (int)ROWS,
                                      start.data(), items.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_assign_features_to_grid: ") + jsorb_last_error(ex.handle()));
    for (std::size_t i = 0; i < COLS; i++)
        for (std::size_t j = 0; j < ROWS; j++) {
            const std::size_t c = i * ROWS + j;
            mGrid[i][j].assign(items.begin() + start[c], items.begin() + start[c + 1]);
        }
}

// Tracking::SearchLocalPoints' matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th) (Tracking.cpp:1782-1791, ORBmatcher.cpp:32-116) on
// the device, over the SAME SyncedMem buffers compute_isInFrustum_GPU just filled (no copy back of u, v, invz, predictedlevel, viewCos,
// isinfrustum): descriptors holds the map points' descriptors (32 bytes each, map_points order), u_right_gpu mvuRight on the device
// (jsorb_stereo_uright_device / jsorb_rgbd_uright_device; nullptr: monocular), blocked_gpu one byte per keypoint (F.mvpMapPoints[k] with
// observations; nullptr: none).  Returns nmatches; match_kp[i] = keypoint matched to map_points[i] or -1 - the caller applies
// mCurrentFrame.mvpMapPoints[match_kp[i]] = map_points[i].
inline int SearchLocalPoints(ORBExtractor &ex, const jsorb_search_params &params, int n_points, SyncedMem<float> &u, SyncedMem<float> &v,
                             SyncedMem<float> &invz, SyncedMem<int> &predictedlevel, SyncedMem<float> &viewCos, SyncedMem<unsigned char> &isinfrustum,
                             SyncedMem<unsigned char> &descriptors, const float *u_right_gpu, const unsigned char *blocked_gpu, std::vector<int> &match_kp)
{
    match_kp.assign(n_points > 0 ? n_points : 1, -1);
    int n_matches = 0;
    if (jsorb_search_local_points(ex.handle(), 0, &params, n_points, u.gpu_data(), v.gpu_data(), invz.gpu_data(), predictedlevel.gpu_data(),
                                  viewCos.gpu_data(), isinfrustum.gpu_data(), descriptors.gpu_data(), u_right_gpu, blocked_gpu, match_kp.data(),
                                  &n_matches) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_local_points: ") + jsorb_last_error(ex.handle()));
    match_kp.resize(n_points > 0 ? n_points : 0);
    return n_matches;
}

// Tracking::UpdateLocalPoints (Tracking.cpp:1818-1841) and the front half of SearchLocalPoints - the frame marks (:1352-1367), map_points
// (:1410-1420), the gathers, the uploads and compute_isInFrustum_GPU (:1427-1600) - in one call on the extractor's stream: kf_start (host) and
// kf_point_row_gpu are mvpLocalKeyFrames' GetMapPointMatches() as table rows, concatenated; frame_point_row_gpu mCurrentFrame.mvpMapPoints as rows
// (nullptr: none).  Returns nToMatch; out feeds SearchLocalPoints(ex, params, out) below.  The host keeps IncreaseVisible over out.point_row,
// mbTrackInView and applying the matches.
inline int UpdateLocalPoints(ORBExtractor &ex, const jsorb::MapPointTable &table, const jsorb_frustum_params &frustum, const std::vector<int32_t> &kf_start,
                             const int32_t *kf_point_row_gpu, const int32_t *frame_point_row_gpu, int capacity, jsorb::LocalMapPoints &out)
{
    const int n = jsorb_n_keypoints(ex.handle(), 0), cap = capacity > 0 ? capacity : 1;
    out.capacity = capacity;
    out.u.resize(cap); out.v.resize(cap); out.invz.resize(cap); out.viewCos.resize(cap); out.predictedlevel.resize(cap); out.point_row_gpu.resize(cap);
    out.isinfrustum.resize(cap); out.descriptors.resize(32 * cap); out.blocked.resize(n > 0 ? n : 1);
    out.point_row.assign(cap, -1);
    const jsorb_map_point_table t = table.view();
    if (jsorb_local_map_points(ex.handle(), 0, &t, &frustum, kf_start.empty() ? 0 : (int)kf_start.size() - 1, kf_start.data(), kf_point_row_gpu, frame_point_row_gpu, capacity,
                               out.point_row_gpu.gpu_data(), out.u.gpu_data(), out.v.gpu_data(), out.invz.gpu_data(), out.predictedlevel.gpu_data(),
                               out.viewCos.gpu_data(), out.isinfrustum.gpu_data(), out.descriptors.gpu_data(), out.blocked.gpu_data(), nullptr,
                               out.point_row.data(), out.counts) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_local_map_points: ") + jsorb_last_error(ex.handle()));
    out.point_row.resize(capacity > 0 ? capacity : 0);
    return out.counts[2];
}
// Tracking::UpdateLocalKeyFrames (Tracking.cpp:1844-1952) on the device: the votes of the frame's map points (frame_rows_gpu,
// mCurrentFrame.mvpMapPoints as table rows, n_frame of them; nullptr: none), the first list, the expansion over neighbours, children and parents,
// and the keyframes' rows concatenated into local.point_row_gpu.  local carries mvpLocalKeyFrames and mpReferenceKF from frame to frame, as the
// reference does when no keyframe gets a vote.  Returns the number of local keyframes; the binding sets mpReferenceKF = slot_to_kf[local.ref_slot].
inline int UpdateLocalKeyFrames(ORBExtractor &ex, const jsorb::KeyframeGraph &graph, const jsorb::MapPointTable &table, const int32_t *frame_rows_gpu,
                                int n_frame, jsorb::LocalKeyFrames &local)
{
    const jsorb_keyframe_graph g = graph.view();
    const jsorb_map_point_table t = table.view();
    local.slots.assign(local.kf_capacity, -1);
    int32_t state[2] = {0, -1};
    if (jsorb_local_keyframes(ex.handle(), &g, &t, frame_rows_gpu, n_frame, local.kf_capacity, local.entry_capacity, local.slot_gpu.gpu_data(),
                              local.state_gpu.gpu_data(), local.start_gpu.gpu_data(), local.point_row_gpu.gpu_data(), local.counts_gpu.gpu_data(),
                              local.slots.data(), state, local.counts) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_local_keyframes: ") + jsorb_last_error(ex.handle()));
    local.slots.resize(state[0]);
    local.ref_slot = state[1];
    return state[0];
}
// KeyFrame::UpdateConnections (KeyFrame.cpp:293-383) of the keyframes `slots` (at most 32) one after the other on the matcher's stream: the maps,
// the ordered lists and the graph's neighbours rows follow on the device; result.parent says whose child a keyframe with its first connection
// becomes.  Returns the keyframes processed.
inline int UpdateConnections(jsorb::KeyframeMatcher &matcher, const jsorb::KeyframeGraph &graph, const jsorb::MapPointTable &table, jsorb::Covisibility &cov,
                             const std::vector<int32_t> &slots, jsorb::UpdatedConnections &result)
{
    const jsorb_keyframe_graph g = graph.view();
    const jsorb_map_point_table t = table.view();
    const int n = (int)slots.size();
    jsorb::DeviceInts dev(2 * (size_t)n + 9);     // the slots, the counts, parent_out
    int32_t *d = dev.p;
    if (n > 0 && jsorb_mem_h2d(d, slots.data(), (size_t)n * sizeof(int32_t)) != JSORB_OK) throw std::runtime_error("UpdateConnections: upload failed");
    result.parent.assign(n > 0 ? n : 1, -1);
    if (jsorb_update_connections(matcher.handle(), &g, &t, &cov.view(), n, d, const_cast<int32_t *>(g.neighbours), d + n + 8, nullptr, d + n,
                                 result.parent.data(), result.counts) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_update_connections: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    result.parent.resize(n);
    return result.counts[0];
}
// SetBadFlag's EraseConnection walk (KeyFrame.cpp:470-471, :480-481) for `slot`; returns the maps that held it.  It waits for the matcher.
inline int EraseConnections(jsorb::KeyframeMatcher &matcher, const jsorb::KeyframeGraph &graph, jsorb::Covisibility &cov, int slot)
{
    const jsorb_keyframe_graph g = graph.view();
    jsorb::DeviceInts counts(2);
    if (jsorb_erase_connections_async(matcher.handle(), &g, &cov.view(), slot, const_cast<int32_t *>(g.neighbours), counts.p) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_erase_connections: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    int32_t h[2] = {0, 0};
    if (jsorb_mem_stream_sync(matcher.stream()) != JSORB_OK || jsorb_mem_d2h(h, counts.p, sizeof(h)) != JSORB_OK)
        throw std::runtime_error("EraseConnections: copy back failed");
    return h[1];
}
// ORBmatcher::Fuse with its map mutations (ORBmatcher.cpp:812-1087, MapPoint.cpp:208-246) for all `targets` (slots) in order, on the device state:
// one direction of LocalMapping::SearchInNeighbors (prm.check_reprojection = 1), or LoopClosing::SearchAndFuse's calls with their Replace loop
// (check_reprojection = 0, replace_loop).  list: the points' table rows, -1 = NULL.  Returns the number of fused points.  The host objects follow
// from result.events and state.replaced(); Map::EraseMapPoint and UpdateNormalAndDepth stay with the caller.
inline int FuseMap(jsorb::KeyframeMatcher &matcher, const jsorb_fuse_params &prm, const jsorb::KeyframeGraph &graph, const jsorb::MapPointTable &table,
                   const jsorb::KeyframeKeypoints &kp, jsorb::FuseState &state, const std::vector<int32_t> &list, const std::vector<int32_t> &targets,
                   const jsorb::FusePoses &poses, jsorb::FusedMap &result, bool replace_loop = false)
{
    const size_t n = list.size(), T = targets.size(), pairs = n * T, cap = pairs ? pairs : 1;
    if (T && (!poses.Rcw || !poses.tcw || !poses.Ow)) throw std::runtime_error("FuseMap: 9 + 3 + 3 pose floats per target (host arrays, as for Fuse)");
    jsorb::DeviceInts dl(n), out(3 * pairs + T + 4 * cap + 10);
    if (n && jsorb_mem_h2d(dl.p, list.data(), n * sizeof(int32_t)) != JSORB_OK) throw std::runtime_error("FuseMap: upload failed");
    int32_t *bi = out.p, *bd = bi + pairs, *rp = bd + pairs, *nf = rp + pairs, *lg = nf + T, *cn = lg + 4 * cap;
    const jsorb_keyframe_graph g = graph.view();
    const jsorb_map_point_table t = table.view();
    const jsorb_keyframe_keypoints k = kp.view();
    result.best_idx.assign(pairs, -1); result.best_dist.assign(pairs, -1); result.replace_point.assign(pairs, -1); result.n_fused.assign(T, 0);
    std::vector<int32_t> log(4 * cap, -1);
    const int rc = jsorb_fuse_map(matcher.handle(), &prm, replace_loop ? 1 : 0, &g, &t, &k, &state.view(), (int)n, dl.p, (int)T, targets.data(), poses.Rcw,
                                  poses.tcw, poses.Ow, bi, bd, rp, nf, (int)cap, lg, cn, result.best_idx.data(), result.best_dist.data(),
                                  result.replace_point.data(), result.n_fused.data(), log.data(), result.counts);
    if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb_fuse_map: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    result.events.clear();
    for (size_t i = 0; i < cap && log[4 * i] >= 0; i++) result.events.push_back({log[4 * i], log[4 * i + 1], log[4 * i + 2], log[4 * i + 3]});
    return result.counts[0];
}

// The loop of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:243-457) for the keyframe in `current_slot` (n1 keypoints) and ALL `neighbours`
// (slots in GetBestCovisibilityKeyFrames order, after the caller's baseline tests) on the device state: matching, triangulation, the gates, and for
// every accepted pair the new row with its two observations, descriptor, normal and distance range.  poses: 1 + neighbours records, the current
// keyframe first; F12, epipole: 9 and 2 floats per neighbour as for SearchForTriangulation; new_rows: the free table rows in the order they are to
// be used.  A keypoint belongs to the first neighbour whose pair is accepted (the reference's loop gives the same: ORBmatcher.cpp:686-690).
// Returns the points created.  The host objects follow from result.created.
inline int CreateNewMapPoints(jsorb::KeyframeMatcher &matcher, const jsorb_triangulation_params &prm, const jsorb::KeyframeGraph &graph,
                              const jsorb::MapPointTable &table, const jsorb::KeyframeKeypoints &kp, const jsorb::NewPointKeypoints &extra,
                              jsorb::NewPointState &state, int current_slot, int n1, int run_capacity, const std::vector<int32_t> &neighbours,
                              const std::vector<jsorb_keyframe_pose> &poses, const float *F12, const float *epipole, float ratio_factor, int current_kf_id,
                              const std::vector<int32_t> &new_rows, jsorb::NewMapPoints &result)
{
    const size_t T = neighbours.size(), pairs = T * (size_t)(n1 > 0 ? n1 : 0), R = new_rows.size(), cap = R ? R : 1;
    if (poses.size() != T + 1 || (T && (!F12 || !epipole))) throw std::runtime_error("CreateNewMapPoints: 1 + T poses, 9 F12 and 2 epipole floats per neighbour");
    if (n1 != graph.point_length(current_slot)) throw std::runtime_error("CreateNewMapPoints: n1 is not the length of the current keyframe's run");
    jsorb::DeviceInts rows(R), out(pairs + 3 * pairs + (pairs + 3) / 4 + 4 * cap + 12);
    if (R && jsorb_mem_h2d(rows.p, new_rows.data(), R * sizeof(int32_t)) != JSORB_OK) throw std::runtime_error("CreateNewMapPoints: upload failed");
    int32_t *vd = out.p, *lg = vd + pairs + 3 * pairs, *cn = lg + 4 * cap;
    float *x3 = reinterpret_cast<float *>(vd + pairs);
    uint8_t *pt = reinterpret_cast<uint8_t *>(cn + 12);
    const jsorb_keyframe_graph g = graph.view();
    const jsorb_map_point_table t = table.view();
    const jsorb_keyframe_keypoints k = kp.view();
    const jsorb_new_point_keypoints e = extra.view();
    result.verdict.assign(pairs, 0); result.path.assign(pairs, 0); result.x3D.assign(3 * pairs, 0.0f);
    std::vector<int32_t> log(4 * cap, -1);
    const int rc = jsorb_create_new_map_points(matcher.handle(), &prm, &g, &t, &k, &e, &state.view(), current_slot, n1, run_capacity, (int)T, neighbours.data(),
                                               poses.data(), F12, epipole, ratio_factor, current_kf_id, (int)R, rows.p, (int)cap, vd, pt, x3, lg, cn,
                                               result.verdict.data(), result.path.data(), result.x3D.data(), log.data(), result.counts);
    if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb_create_new_map_points: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    result.created.clear();
    for (size_t i = 0; i < cap && log[4 * i + 1] >= 0; i++)
        if (log[4 * i] >= 0) result.created.push_back({log[4 * i], log[4 * i + 1], log[4 * i + 2], log[4 * i + 3]});
    return result.counts[3];
}

// LocalMapping::KeyFrameCulling (LocalMapping.cpp:638-702) for the current keyframe, with the whole of SetBadFlag (KeyFrame.cpp:457-549) for every
// keyframe it culls, on the matcher's stream: the candidates are the current keyframe's ordered list read on the device, and the call is repeated
// past its 4 culls until the list is done.  first_slot: the slot of keyframe 0 (-1: none).  What stays with the binding afterwards: the child
// runs (graph.set_children from result.reparent), mTcp, Map::EraseKeyFrame and KeyframeDatabase::erase for result.culled.  Returns the culled.
inline int KeyFrameCulling(jsorb::KeyframeMatcher &matcher, const jsorb::KeyframeGraph &graph, const jsorb::MapPointTable &table, jsorb::Covisibility &cov,
                           const jsorb::KeyframeViews &views, jsorb::CullingState &state, int current_slot, bool monocular, jsorb::CulledKeyFrames &result,
                           int first_slot = -1)
{
    const jsorb_keyframe_graph g = graph.view();
    const jsorb_map_point_table t = table.view();
    const jsorb_keyframe_views v = views.view();
    const int C = cov.conn_capacity(), S = cov.max_keyframes(), max_cull = 4, cap = S > (1 << 21) ? (1 << 23) : max_cull * (S > 0 ? S : 1);      // (every round is enqueued whether it culls or not: four per call, and the loop below goes on)
    jsorb::DeviceInts dev((size_t)4 * C + 2 + max_cull + 2 * (size_t)cap + 10);
    int32_t *cand = dev.p, *len = cand + C, *slot = len + 1, *decision = slot + 1, *n_mps = decision + C, *n_red = n_mps + C, *culled = n_red + C,
            *reparent = culled + max_cull, *counts = reparent + 2 * (size_t)cap;
    const int32_t cur = current_slot;
    int32_t n = 0;
    if (jsorb_mem_h2d(slot, &cur, sizeof(cur)) != JSORB_OK) throw std::runtime_error("KeyFrameCulling: upload failed");
    if (jsorb_best_covisibles_async(matcher.handle(), &cov.view(), 1, slot, C, cand, len) != JSORB_OK)       // the copy of :644
        throw std::runtime_error(std::string("jsorb_best_covisibles: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    if (jsorb_mem_stream_sync(matcher.stream()) != JSORB_OK || jsorb_mem_d2h(&n, len, sizeof(n)) != JSORB_OK) throw std::runtime_error("KeyFrameCulling: copy back failed");
    result = jsorb::CulledKeyFrames();
    result.candidates.resize(n); result.decision.assign(n, -1); result.n_mps.assign(n, 0); result.n_redundant.assign(n, 0);
    if (n > 0 && jsorb_mem_d2h(result.candidates.data(), cand, (size_t)n * sizeof(int32_t)) != JSORB_OK) throw std::runtime_error("KeyFrameCulling: copy back failed");
    std::vector<int32_t> h_culled(max_cull), h_rep(2 * (size_t)cap);
    int done = 0;
    while (done < n) {
        int32_t c[10];
        if (jsorb_cull_keyframes(matcher.handle(), &g, &t, &cov.view(), &v, &state.view(), monocular ? 1 : 0, first_slot, n - done, cand + done, max_cull,
                                 const_cast<int32_t *>(g.neighbours), cap, decision, n_mps, n_red, culled, reparent, counts, result.decision.data() + done,
                                 result.n_mps.data() + done, result.n_redundant.data() + done, h_culled.data(), h_rep.data(), c) != JSORB_OK)
            throw std::runtime_error(std::string("jsorb_cull_keyframes: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
        if (c[9] != 0) throw std::runtime_error("KeyFrameCulling: the reparent log overflowed");      // (a cull hands on at most S children: not reached)
        for (int i = 0; i < max_cull && h_culled[i] >= 0; i++) result.culled.push_back(h_culled[i]);
        for (int i = 0; i < c[8] && i < cap; i++) result.reparent.push_back({h_rep[2 * i], h_rep[2 * i + 1]});
        for (int i = 1; i < 10; i++) result.counts[i] += c[i];
        if (c[0] <= 0) break;                    // (every call decides at least one candidate)
        done += c[0];
    }
    result.counts[0] = n;
    return (int)result.culled.size();
}
// The getters of KeyFrame.cpp:163-212 over one slot's copy, as slots; argument orders as the reference's
inline std::vector<int32_t> GetConnectedKeyFrames(const jsorb::Covisibility &cov, int slot) { return cov.copy(slot).conn_slot; }
inline std::vector<int32_t> GetVectorCovisibleKeyFrames(const jsorb::Covisibility &cov, int slot) { return cov.copy(slot).ord_slot; }
inline std::vector<int32_t> GetBestCovisibilityKeyFrames(const jsorb::Covisibility &cov, int slot, int N)
{
    std::vector<int32_t> v = cov.copy(slot).ord_slot;
    if ((int)v.size() > N) v.resize(N > 0 ? N : 0);
    return v;
}
inline std::vector<int32_t> GetCovisiblesByWeight(const jsorb::Covisibility &cov, int slot, int w)
{
    const jsorb::Covisibility::Slot s = cov.copy(slot);
    size_t n = 0;                                // upper_bound with weightComp (a > b): the first weight below w
    while (n < s.ord_weight.size() && s.ord_weight[n] >= w) n++;
    if (s.ord_slot.empty() || n == s.ord_weight.size()) return {};       // :192-197: empty when every weight is at or above w
    return std::vector<int32_t>(s.ord_slot.begin(), s.ord_slot.begin() + n);
}
inline int GetWeight(const jsorb::Covisibility &cov, int slot, int other)
{
    const jsorb::Covisibility::Slot s = cov.copy(slot);
    for (size_t i = 0; i < s.conn_slot.size(); i++)
        if (s.conn_slot[i] == other) return s.conn_weight[i];
    return 0;
}
// ... and UpdateLocalPoints over that list: ONE keyframe of local.entry_capacity entries, the padding behind the last row dropped as NULL entries
inline int UpdateLocalPoints(ORBExtractor &ex, const jsorb::MapPointTable &table, const jsorb_frustum_params &frustum, jsorb::LocalKeyFrames &local,
                             const int32_t *frame_rows_gpu, int capacity, jsorb::LocalMapPoints &pts)
{
    return UpdateLocalPoints(ex, table, frustum, std::vector<int32_t>{0, local.entry_capacity}, local.point_row_gpu.gpu_data(), frame_rows_gpu, capacity, pts);
}
// ... and the matcher over those slots: match_kp[i] = the keypoint matched to the map point of row out.point_row[i], or -1
inline int SearchLocalPoints(ORBExtractor &ex, const jsorb_search_params &params, jsorb::LocalMapPoints &pts, const float *u_right_gpu, std::vector<int> &match_kp)
{
    return SearchLocalPoints(ex, params, pts.capacity, pts.u, pts.v, pts.invz, pts.predictedlevel, pts.viewCos, pts.isinfrustum, pts.descriptors, u_right_gpu,
                             pts.blocked.gpu_data(), match_kp);
}

// F.mvpMapPoints[bestIdx] = pMP (ORBmatcher.cpp:107) on the device, enqueued on the extractor's stream: frame_point_row_gpu[match_kp_gpu[i]] =
// point_row_gpu[i] for the matches of a matcher whose match_kp stayed on the device (jsorb_search_local_points_async over pts: point_row_gpu =
// pts.point_row_gpu).  frame_point_row_gpu: one row per keypoint of the frame, -1 = NULL.
inline void ApplyMatches(ORBExtractor &ex, int n_points, const int32_t *point_row_gpu, const int32_t *match_kp_gpu, int32_t *frame_point_row_gpu)
{
    if (jsorb_apply_matches_async(jsorb_get_stream(ex.handle()), n_points, point_row_gpu, match_kp_gpu, jsorb_n_keypoints(ex.handle(), 0), frame_point_row_gpu) != JSORB_OK)
        throw std::runtime_error("jsorb_apply_matches_async failed");
}
// Optimizer::PoseOptimization(&mCurrentFrame) (Optimizer.cpp:244-456; Tracking.cpp:937, :1077, :1140) on the device: frame_point_row_gpu is
// mCurrentFrame.mvpMapPoints as table rows (-1 = NULL), u_right_gpu mvuRight on the device (nullptr: monocular), Tcw mTcw row-major - read, and
// written as SetPose(pose) does.  outlier = mvbOutlier (one byte per keypoint).  point_row_out_gpu (or nullptr): the rows with the outliers' set to
// -1, the discard of Tracking.cpp:1086-1103.  Returns the reference's int: nInitialCorrespondences - nBad, 0 with fewer than 3 correspondences.
inline int PoseOptimization(ORBExtractor &ex, const jsorb::MapPointTable &table, const int32_t *frame_point_row_gpu, float Tcw[16],
                            std::vector<unsigned char> &outlier, const jsorb::PoseParams &prm, const float *u_right_gpu = nullptr,
                            int32_t *point_row_out_gpu = nullptr, int32_t counts[4] = nullptr)
{
    const int N = jsorb_n_keypoints(ex.handle(), 0);
    outlier.assign(N > 0 ? N : 1, 0);
    const jsorb_map_point_table t = table.view();
    float out[16];
    int32_t c[4] = {0, 0, 0, 0};
    if (jsorb_pose_optimization(ex.handle(), 0, &prm, &t, 1, frame_point_row_gpu, u_right_gpu, Tcw, out, nullptr, outlier.data(), point_row_out_gpu, c) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_pose_optimization: ") + jsorb_last_error(ex.handle()));
    outlier.resize(N > 0 ? N : 0);
    for (int i = 0; i < 16; i++) Tcw[i] = out[i];
    if (counts) for (int i = 0; i < 4; i++) counts[i] = c[i];
    return c[2];
}

// TrackWithMotionModel's matcher.SearchByProjection(mCurrentFrame, mLastFrame, th, bMono) and its retry at 2 th (Tracking.cpp:1045-1064,
// ORBmatcher.cpp:1647-1963) on the device, in one call: Px / Py / Pz hold GetWorldPosExp of the last frame's map points that are not outliers
// (ascending last-frame index), octave / angle the last frame's mvKeys[].octave and mvKeysUn[].angle of those keypoints, descriptors their
// GetDescriptorExp rows (32 bytes each); u_right_gpu mvuRight on the device (jsorb_stereo_uright_device / jsorb_rgbd_uright_device; nullptr:
// monocular).  The buffers are read on the device: upload them (to_gpu) first.  Returns nmatches; kp_match[k] = index of the point now in
// mCurrentFrame.mvpMapPoints[k] or -1 - the caller applies mvpMapPoints[k] = points[kp_match[k]].
inline int SearchLastFrame(ORBExtractor &ex, const jsorb_last_frame_params &params, int n_points, SyncedMem<float> &Px, SyncedMem<float> &Py,
                           SyncedMem<float> &Pz, SyncedMem<int> &octave, SyncedMem<float> &angle, SyncedMem<unsigned char> &descriptors,
                           const float *u_right_gpu, std::vector<int> &kp_match)
{
    const int N = jsorb_n_keypoints(ex.handle(), 0);
    kp_match.assign(N > 0 ? N : 1, -1);
    int n_matches = 0;
    if (jsorb_search_last_frame(ex.handle(), 0, &params, n_points, Px.gpu_data(), Py.gpu_data(), Pz.gpu_data(), octave.gpu_data(), angle.gpu_data(),
                                descriptors.gpu_data(), u_right_gpu, kp_match.data(), &n_matches) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_last_frame: ") + jsorb_last_error(ex.handle()));
    kp_match.resize(N > 0 ? N : 0);
    return n_matches;
}

// MonocularInitialization's matcher.SearchForInitialization(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches, windowSize)
// (Tracking.cpp:724-794, ORBmatcher.cpp:392-507) on the device.  KeepInitialFrame right after the extract that becomes mInitialFrame (where the
// reference fills mvbPrevMatched from mvKeysUn, Tracking.cpp:735-737): the extractor keeps that frame's octaves, angles, descriptors and
// mvbPrevMatched on the device across the following extracts.  SearchForInitialization after every later extract: returns nmatches, vnMatches12[i1]
// = keypoint of the current frame matched to keypoint i1 of the initial frame or -1, and (when asked for) the updated mvbPrevMatched as x[n1]
// then y[n1].  DropInitialFrame where the reference deletes mpInitializer.
inline int KeepInitialFrame(ORBExtractor &ex)
{
    if (jsorb_init_reference_set(ex.handle(), 0) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_init_reference_set: ") + jsorb_last_error(ex.handle()));
    return jsorb_init_reference_n(ex.handle());
}
inline void DropInitialFrame(ORBExtractor &ex) { jsorb_init_reference_clear(ex.handle()); }
inline int SearchForInitialization(ORBExtractor &ex, const jsorb_init_params &params, std::vector<int> &vnMatches12,
                                   std::vector<float> *vbPrevMatched = nullptr)
{
    const int n1 = jsorb_init_reference_n(ex.handle());
    vnMatches12.assign(n1 > 0 ? n1 : 1, -1);
    if (vbPrevMatched) vbPrevMatched->assign(n1 > 0 ? 2 * (std::size_t)n1 : 1, 0.0f);
    int n_matches = 0;
    if (jsorb_search_initial_frame(ex.handle(), 0, &params, vnMatches12.data(), vbPrevMatched ? vbPrevMatched->data() : nullptr, &n_matches) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_initial_frame: ") + jsorb_last_error(ex.handle()));
    vnMatches12.resize(n1 > 0 ? n1 : 0);
    if (vbPrevMatched) vbPrevMatched->resize(n1 > 0 ? 2 * (std::size_t)n1 : 0);
    return n_matches;
}

// The bag-of-words side of TrackReferenceKeyFrame (Tracking.cpp:919-932) and Relocalization (:1954-2004) on the device.
// ComputeBoW after the extract, where the reference calls mCurrentFrame.ComputeBoW() (Frame.cpp:709-716): word and node ids of every keypoint stay
// on the device for SearchByBoW; asked for on the host, the caller folds them into mBowVec (addWeight / addIfNotExist with the vocabulary's own
// weights, in feature order) and mFeatVec (addFeature(node_id[i], i) for node_id[i] >= 0).
inline void ComputeBoW(ORBExtractor &ex, const jsorb::Vocabulary &voc, std::vector<int> *word_id = nullptr, std::vector<int> *node_id = nullptr)
{
    if (jsorb_bow_transform_async(ex.handle(), 0, voc.handle()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_bow_transform_async: ") + jsorb_last_error(ex.handle()));
    if (!word_id && !node_id) return;
    const int N = jsorb_n_keypoints(ex.handle(), 0);
    if (word_id) word_id->assign(N > 0 ? N : 1, -1);
    if (node_id) node_id->assign(N > 0 ? N : 1, -1);
    if (jsorb_copy_bow(ex.handle(), 0, word_id ? word_id->data() : nullptr, node_id ? node_id->data() : nullptr) != JSORB_OK)
        throw std::runtime_error("jsorb_copy_bow failed");
    if (word_id) word_id->resize(N > 0 ? N : 0);
    if (node_id) node_id->resize(N > 0 ? N : 0);
}
// matcher.SearchByBoW(pKF, mCurrentFrame, vpMapPointMatches) (ORBmatcher.cpp:146-275) for one keyframe of n keypoints against the current frame,
// after ComputeBoW: node = the keyframe's FeatureVector node per keypoint (-1: none), valid = pMP && !pMP->isBad(), angle = mvKeysUn[].angle,
// descriptors 32 bytes each, uploaded (to_gpu) by the caller.  Returns nmatches; match_kf[k] = the keyframe keypoint whose map point is now in
// vpMapPointMatches[k], or -1 - the caller applies vpMapPointMatches[k] = vpMapPointsKF[match_kf[k]].
inline int SearchByBoW(ORBExtractor &ex, const jsorb_bow_params &params, int n, SyncedMem<int> &node, SyncedMem<unsigned char> &valid,
                       SyncedMem<float> &angle, SyncedMem<unsigned char> &descriptors, std::vector<int> &match_kf)
{
    const int N = jsorb_n_keypoints(ex.handle(), 0);
    match_kf.assign(N > 0 ? N : 1, -1);
    const int32_t kf_start[2] = {0, n};
    int n_matches = 0;
    if (jsorb_search_by_bow(ex.handle(), 0, &params, nullptr, 1, kf_start, node.gpu_data(), valid.gpu_data(), angle.gpu_data(), descriptors.gpu_data(),
                            match_kf.data(), &n_matches) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_by_bow: ") + jsorb_last_error(ex.handle()));
    match_kf.resize(N > 0 ? N : 0);
    return n_matches;
}

// matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false) (ORBmatcher.cpp:644-810) for ALL n_kf neighbours of
// LocalMapping::CreateNewMapPoints' loop (LocalMapping.cpp:243-275) in one call: kf2 holds the neighbours concatenated, neighbour i at
// kf_start[i] .. kf_start[i + 1]; F12s 9 floats (row-major ComputeF12) and epipoles 2 floats (ex, ey of :651-657) per neighbour, on the host.
// vMatchedPairs[i] is the reference's vMatchedPairs for neighbour i ((idx1, idx2) with idx2 local to the neighbour, ascending idx1); returns the
// reference's return value per neighbour.
inline std::vector<int> SearchForTriangulation(jsorb::KeyframeMatcher &matcher, const jsorb_triangulation_params &params, const jsorb::KeyframeSide &kf1,
                                               int n_kf, const int32_t *kf_start, const jsorb::KeyframeSide &kf2, const float *F12s, const float *epipoles,
                                               std::vector<std::vector<std::pair<size_t, size_t>>> &vMatchedPairs)
{
    std::vector<int32_t> match12((size_t)(n_kf > 0 ? n_kf : 0) * (kf1.n > 0 ? kf1.n : 0) + 1, -1);
    std::vector<int> counts(n_kf > 0 ? n_kf : 1, 0);
    if (jsorb_search_for_triangulation(matcher.handle(), &params, kf1.n, kf1.node, kf1.is_free, kf1.stereo, kf1.x, kf1.y, kf1.angle, kf1.descriptors, n_kf,
                                       kf_start, kf2.node, kf2.is_free, kf2.stereo, kf2.x, kf2.y, kf2.octave, kf2.angle, kf2.descriptors, F12s, epipoles,
                                       match12.data(), counts.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_for_triangulation: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    counts.resize(n_kf > 0 ? n_kf : 0);
    vMatchedPairs.assign(counts.size(), {});
    for (size_t i = 0; i < counts.size(); i++) {
        vMatchedPairs[i].reserve(counts[i] > 0 ? counts[i] : 0);
        for (int k = 0; k < kf1.n; k++)
            if (match12[i * kf1.n + k] >= 0) vMatchedPairs[i].push_back(std::make_pair((size_t)k, (size_t)match12[i * kf1.n + k]));
    }
    return counts;
}

// The search of matcher.Fuse(pKFi, vpMapPointMatches) (ORBmatcher.cpp:812-936; with params.check_reprojection = 0 the loop-closing overload
// :964-1087) for ALL n_kf target keyframes of LocalMapping::SearchInNeighbors' loops (LocalMapping.cpp:460-540) in one call: keyframes holds the
// targets concatenated, target k at kf_start[k] .. kf_start[k + 1].  skip_gpu: nullptr or one byte per (keyframe, point) on the device, nonzero
// where the caller already knows the head test fails (!pMP, isBad, IsInKeyFrame).  best_idx / best_dist [k * points.n + i] = bestIdx (within
// keyframe k) and bestDist of point i, -1 where the reference finds none within TH_LOW.  The caller replays the head test and the tail :938-958
// over them, keyframes and points in the reference's order, and calls this again - for the keyframes not yet replayed - for every point whose
// descriptor a Replace changed (MapPoint.cpp:243 recomputes the survivor's; include/jsorb.h).  Returns the number of matches over
// all keyframes.
inline int Fuse(jsorb::KeyframeMatcher &matcher, const jsorb_fuse_params &params, const jsorb::FusePoints &points, int n_kf, const int32_t *kf_start,
                const jsorb::FuseKeyframes &keyframes, const jsorb::FusePoses &poses, const unsigned char *skip_gpu, std::vector<int32_t> &best_idx,
                std::vector<int32_t> &best_dist)
{
    const size_t rows = (size_t)(n_kf > 0 ? n_kf : 0) * (points.n > 0 ? points.n : 0);
    best_idx.assign(rows + 1, -1);
    best_dist.assign(rows + 1, -1);
    std::vector<int> counts(n_kf > 0 ? n_kf : 1, 0);
    if (jsorb_fuse(matcher.handle(), &params, points.n, points.Px, points.Py, points.Pz, points.Nx, points.Ny, points.Nz, points.max_distance,
                   points.min_dist_inv, points.max_dist_inv, points.descriptors, n_kf, kf_start, keyframes.x, keyframes.y, keyframes.octave,
                   keyframes.uright, keyframes.descriptors, poses.Rcw, poses.tcw, poses.Ow, skip_gpu, best_idx.data(), best_dist.data(),
                   counts.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_fuse: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    best_idx.resize(rows);
    best_dist.resize(rows);
    int total = 0;
    for (int k = 0; k < n_kf; k++) total += counts[k];
    return total;
}

// pMP->ComputeDistinctiveDescriptors() (MapPoint.cpp:273-338) for ALL the points LocalMapping touches at one place - ProcessNewKeyFrame
// (LocalMapping.cpp:158-159), CreateNewMapPoints (:448), SearchInNeighbors (:532), the survivors of MapPoint::Replace (MapPoint.cpp:243) - in one
// call.  table_gpu: nullptr or the device table of the map points' descriptors (n_table_rows x 32 bytes, the `desc` a following Fuse reads):
// the row of every point with an observation is overwritten with the winner's bytes, the others keep theirs (:287, :300).  changed_gpu: nullptr
// or obs.n bytes on the device, 1 where a row got other bytes than it held - the points to search again after a replay (include/jsorb.h).
// best_obs[p] = BestIdx within the point's own list or -1, best_median[p] its median or -1.  Returns the number of points with a winner.
inline int ComputeDistinctiveDescriptors(jsorb::KeyframeMatcher &matcher, const jsorb::Observations &obs, unsigned char *table_gpu, int n_table_rows,
                                         unsigned char *changed_gpu, std::vector<int32_t> &best_obs, std::vector<int32_t> &best_median)
{
    const size_t n = obs.n > 0 ? obs.n : 0;
    best_obs.assign(n + 1, -1);
    best_median.assign(n + 1, -1);
    if (jsorb_distinctive_descriptors(matcher.handle(), obs.n, obs.obs_start, obs.n_obs, obs.obs_row, obs.kf_descriptors, obs.n_rows, obs.out_row,
                                      n_table_rows, table_gpu, changed_gpu, best_obs.data(), best_median.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_distinctive_descriptors: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    best_obs.resize(n);
    best_median.resize(n);
    int found = 0;
    for (size_t p = 0; p < n; p++) found += best_obs[p] >= 0;
    return found;
}

// Frame::ComputeBoW / KeyFrame::ComputeBoW's mBowVec (Frame.cpp:393-401) from n word ids on the DEVICE (jsorb_bow_word_device of the frame, behind
// jsorb_bow_transform_async), into `v` - enqueued on the database's stream, nothing waited for.
inline void ComputeBowVector(jsorb::KeyframeDatabase &db, const int32_t *word_id_gpu, int n, const jsorb::DeviceBowVector &v)
{
    if (v.cap < n) throw std::invalid_argument("ComputeBowVector: the vector's capacity is below n");
    db.check(jsorb_bow_vector_async(db.handle(), word_id_gpu, n, v.word, v.value, v.n), "bow_vector");
}

// mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore) (KeyFrameDatabase.cpp:80-201) as slots in the reference's output order.
// connected_gpu: a byte per slot (mpCurrentKF->GetConnectedKeyFrames()) or nullptr; neighbours_gpu: max_keyframes x 10 slots, row s =
// GetBestCovisibilityKeyFrames(10) of slot s, -1 padding (both DEVICE, include/jsorb.h).  min_score_gpu: nullptr, or the device float
// LoopMinScore left (then min_score is not read).
inline std::vector<int> DetectLoopCandidates(jsorb::KeyframeDatabase &db, const jsorb::DeviceBowVector &bow, unsigned long long kf_id,
                                             const unsigned char *connected_gpu, const int32_t *neighbours_gpu, float min_score,
                                             const float *min_score_gpu = nullptr)
{
    std::vector<int32_t> out((size_t)db.max_keyframes());
    int n = 0;
    db.check(jsorb_detect_loop_candidates(db.handle(), bow.word, bow.value, bow.cap, bow.n, kf_id, connected_gpu, neighbours_gpu, min_score, min_score_gpu,
                                          out.data(), &n), "detect_loop_candidates");
    return std::vector<int>(out.begin(), out.begin() + n);
}

// The minScore loop of LoopClosing::DetectLoop (LoopClosing.cpp:129-143) over the covisible keyframes' slots (DEVICE, n_slots of them): the
// minimum lands in *min_score_gpu, which DetectLoopCandidates reads with no wait in between.  score_gpu: n_slots floats.
inline void LoopMinScore(jsorb::KeyframeDatabase &db, const jsorb::DeviceBowVector &bow, const int32_t *slots_gpu, int n_slots, float *score_gpu,
                         float *min_score_gpu)
{
    db.check(jsorb_keyframe_database_score_async(db.handle(), bow.word, bow.value, bow.cap, bow.n, slots_gpu, n_slots, score_gpu, nullptr, min_score_gpu),
             "score");
}

// mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame) (KeyFrameDatabase.cpp:203-313, Tracking.cpp:1961) as slots in its output order
inline std::vector<int> DetectRelocalizationCandidates(jsorb::KeyframeDatabase &db, const jsorb::DeviceBowVector &bow, unsigned long long frame_id,
                                                       const int32_t *neighbours_gpu)
{
    std::vector<int32_t> out((size_t)db.max_keyframes());
    int n = 0;
    db.check(jsorb_detect_relocalization_candidates(db.handle(), bow.word, bow.value, bow.cap, bow.n, frame_id, neighbours_gpu, out.data(), &n),
             "detect_relocalization_candidates");
    return std::vector<int>(out.begin(), out.begin() + n);
}

// matcher.SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) (ORBmatcher.cpp:509-642) for ALL n_kf consistent candidates of
// LoopClosing::ComputeSim3's loop (LoopClosing.cpp:255-285) in one call: candidates holds them concatenated, candidate i at kf_start[i] ..
// kf_start[i + 1].  match12[i][idx1] = the keypoint of candidate i (local to it) whose map point the reference puts into
// vvpMapPointMatches[i][idx1], or -1: the caller writes vpMatches12[idx1] = pKF->GetMapPointMatches()[match12[i][idx1]].  Returns the reference's
// return value per candidate.
inline std::vector<int> SearchByBoW(jsorb::KeyframeMatcher &matcher, const jsorb_bow_params &params, const jsorb::BowKeyframeSide &kf1, int n_kf,
                                    const int32_t *kf_start, const jsorb::BowKeyframeSide &candidates, std::vector<std::vector<int>> &match12)
{
    const size_t n1 = kf1.n > 0 ? kf1.n : 0;
    std::vector<int32_t> rows((size_t)(n_kf > 0 ? n_kf : 0) * n1 + 1, -1);
    std::vector<int> counts(n_kf > 0 ? n_kf : 1, 0);
    if (jsorb_search_by_bow_kf(matcher.handle(), &params, kf1.n, kf1.node, kf1.valid, kf1.angle, kf1.descriptors, n_kf, kf_start, candidates.node,
                               candidates.valid, candidates.angle, candidates.descriptors, rows.data(), counts.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_by_bow_kf: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    counts.resize(n_kf > 0 ? n_kf : 0);
    match12.assign(counts.size(), {});
    for (size_t i = 0; i < counts.size(); i++) match12[i].assign(rows.begin() + i * n1, rows.begin() + (i + 1) * n1);
    return counts;
}

// matcher.SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5) (ORBmatcher.cpp:1089-1313, LoopClosing.cpp:328): side1 / side2 are the two
// keyframes' slots; the caller fills their `search` flags from vpMatches12 as :1116-1129 does and computes sR21, t21, sR12 from cv::Mat as
// :1106-1108 does.  match12[i1] = idx2 where both directions agree, else -1: the caller writes vpMatches12[i1] = vpMapPoints2[idx2] there and leaves
// the rest alone.  Returns nFound.
inline int SearchBySim3(jsorb::KeyframeMatcher &matcher, const jsorb_sim3_params &params, const jsorb::Sim3Side &side1, const jsorb::Sim3Side &side2,
                        std::vector<int> &match12, std::vector<int> *vnMatch1 = nullptr, std::vector<int> *vnMatch2 = nullptr)
{
    match12.assign((side1.n > 0 ? side1.n : 0) + 1, -1);
    if (vnMatch1) vnMatch1->assign((side1.n > 0 ? side1.n : 0) + 1, -1);
    if (vnMatch2) vnMatch2->assign((side2.n > 0 ? side2.n : 0) + 1, -1);
    int found = 0;
    if (jsorb_search_by_sim3(matcher.handle(), &params, &side1, &side2, vnMatch1 ? vnMatch1->data() : nullptr, vnMatch2 ? vnMatch2->data() : nullptr,
                             match12.data(), &found) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_by_sim3: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    match12.resize(side1.n > 0 ? side1.n : 0);
    if (vnMatch1) vnMatch1->resize(match12.size());
    if (vnMatch2) vnMatch2->resize(side2.n > 0 ? side2.n : 0);
    return found;
}

// matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10) (ORBmatcher.cpp:277-390, LoopClosing.cpp:380) in the
// reference's argument shape: Scw 4 x 4 row-major, vpPoints the loop points, vpMatched[k] the point keypoint k holds (nullptr: none; resized to the
// keyframe's keypoints).  Here, as the reference does: Scw decomposed (:286-290), bad points and members of spAlreadyFound dropped (:293-305), and
// vpMatched[bestIdx] = pMP written for every match (:383).  The dropped points are map state, which is why this is host code; the points that
// remain go to the device in one upload and the matches come back in one copy.  params: camera, bounds, grid and levels of the keyframe (th and
// the pose are set here).  Returns nmatches.  (Build the caller without floating-point contraction if Scw is not a scaled rigid motion of
// dyadic numbers: the decomposition is the reference's, term for term, only when no product is fused into a sum.)
inline int SearchByProjection(jsorb::KeyframeMatcher &matcher, jsorb_scw_params params, const jsorb::ScwKeyframe &kf, const float *Scw,
                              const std::vector<const jsorb::ScwPoint *> &vpPoints, std::vector<const jsorb::ScwPoint *> &vpMatched, int th)
{
    const int N = kf.n > 0 ? kf.n : 0;
    vpMatched.resize((size_t)N, nullptr);
    // :286-290
    const float scw = std::sqrt(Scw[0] * Scw[0] + Scw[1] * Scw[1] + Scw[2] * Scw[2]);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) params.Rcw[3 * r + c] = Scw[4 * r + c] / scw;
        params.tcw[r] = Scw[4 * r + 3] / scw;
    }
    for (int c = 0; c < 3; c++) params.Ow[c] = -(params.Rcw[c] * params.tcw[0] + params.Rcw[3 + c] * params.tcw[1] + params.Rcw[6 + c] * params.tcw[2]);
    params.th = (float)th;
    // :293-305
    std::set<const jsorb::ScwPoint *> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(nullptr);
    std::vector<const jsorb::ScwPoint *> searched;
    for (const jsorb::ScwPoint *pMP : vpPoints)
        if (pMP && !pMP->bad && !spAlreadyFound.count(pMP)) searched.push_back(pMP);
    const int n = (int)searched.size();
    // one upload: nine float arrays of n, the descriptors (16-byte aligned), blocked
    const size_t nf = ((size_t)n + 3) / 4 * 4, fl = 9 * nf * sizeof(float), bytes = fl + 32 * (size_t)n + (size_t)N + 16;
    std::vector<unsigned char> host(bytes, 0);
    float *f = reinterpret_cast<float *>(host.data());
    for (int i = 0; i < n; i++) {
        const jsorb::ScwPoint &p = *searched[(size_t)i];
        for (int a = 0; a < 3; a++) { f[a * nf + i] = p.pos[a]; f[(3 + a) * nf + i] = p.normal[a]; }
        f[6 * nf + i] = p.max_distance; f[7 * nf + i] = p.min_dist_inv; f[8 * nf + i] = p.max_dist_inv;
        std::memcpy(host.data() + fl + 32 * (size_t)i, p.descriptor, 32);
    }
    for (int k = 0; k < N; k++) host[fl + 32 * (size_t)n + k] = vpMatched[(size_t)k] != nullptr;
    void *dev = nullptr;
    if (jsorb_mem_alloc_device(bytes, &dev) != JSORB_OK || jsorb_mem_h2d(dev, host.data(), bytes) != JSORB_OK) {
        if (dev) jsorb_mem_free_device(dev);
        throw std::runtime_error(std::string("SearchByProjection: ") + jsorb_mem_last_error());
    }
    const float *d = static_cast<const float *>(dev);
    const unsigned char *db = static_cast<const unsigned char *>(dev) + fl;
    std::vector<int32_t> match_kp((size_t)n + 1, -1), kp_match((size_t)N + 1, -1);
    int found = 0;
    const int rc = jsorb_search_by_projection_sim3(matcher.handle(), &params, n, d, d + nf, d + 2 * nf, d + 3 * nf, d + 4 * nf, d + 5 * nf, d + 6 * nf,
                                                   d + 7 * nf, d + 8 * nf, db, N, kf.x, kf.y, kf.octave, kf.descriptors, db + 32 * (size_t)n,
                                                   match_kp.data(), nullptr, kp_match.data(), &found);
    jsorb_mem_free_device(dev);
    if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb_search_by_projection_sim3: ") + jsorb_keyframe_matcher_last_error(matcher.handle()));
    for (int k = 0; k < N; k++)
        if (kp_match[(size_t)k] >= 0) vpMatched[(size_t)k] = searched[(size_t)kp_match[(size_t)k]];      // :383
    return found;
}

// Relocalization's matcher2.SearchByProjection(mCurrentFrame, vpCandidateKFs[i], sFound, th, ORBdist) (Tracking.cpp:2065 with (10, 100), :2079 with
// (3, 64); ORBmatcher.cpp:1968-2095) on the device.  The caller compacts the keyframe's slots with pMP && !pMP->isBad() && !sFound.count(pMP) in
// ascending slot order: Px / Py / Pz hold GetWorldPos, max_distance mfMaxDistance, max_dist_inv / min_dist_inv GetMaxDistanceInvariance /
// GetMinDistanceInvariance, angle pKF->mvKeysUn[slot].angle and descriptors GetDescriptor (32 bytes each) of those points, uploaded (to_gpu) first;
// blocked_gpu one byte per keypoint of the current frame (mCurrentFrame.mvpMapPoints[k] != NULL before the call; nullptr: none).  params carries
// mCurrentFrame.mTcw, its camera centre, the camera and the grid.  Returns nadditional; kp_match[k] = index (into the compacted points) of the point
// now in mCurrentFrame.mvpMapPoints[k], or -1 where this call put none - the caller applies mvpMapPoints[k] = points[kp_match[k]].
inline int SearchByProjection(ORBExtractor &ex, const jsorb_kf_projection_params &params, int n_points, SyncedMem<float> &Px, SyncedMem<float> &Py,
                              SyncedMem<float> &Pz, SyncedMem<float> &max_distance, SyncedMem<float> &max_dist_inv, SyncedMem<float> &min_dist_inv,
                              SyncedMem<float> &angle, SyncedMem<unsigned char> &descriptors, const unsigned char *blocked_gpu, std::vector<int> &kp_match)
{
    const int N = jsorb_n_keypoints(ex.handle(), 0);
    kp_match.assign(N > 0 ? N : 1, -1);
    int n_matches = 0;
    if (jsorb_search_by_projection_kf(ex.handle(), 0, &params, n_points, Px.gpu_data(), Py.gpu_data(), Pz.gpu_data(), max_distance.gpu_data(),
                                      max_dist_inv.gpu_data(), min_dist_inv.gpu_data(), angle.gpu_data(), descriptors.gpu_data(), blocked_gpu,
                                      kp_match.data(), &n_matches) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_search_by_projection_kf: ") + jsorb_last_error(ex.handle()));
    kp_match.resize(N > 0 ? N : 0);
    return n_matches;
}

// Rectification on the device instead of the host cv::remap of the reference's stereo driver (Examples/Stereo/stereo_euroc.cpp:106-107 build
// M1l/M2l, M1r/M2r with cv::initUndistortRectifyMap; :145-146 remap both images of every frame with INTER_LINEAR): set the maps ONCE per
// extractor, then hand every extract() the raw camera image.  Maps of the extractor's image size, rows dense (width floats apart).
inline void SetRectifyMaps(ORBExtractor &ex, const float *mapx, const float *mapy)
{
    int h = 0, w = 0;
    if (jsorb_level_dims(ex.handle(), 0, &h, &w, nullptr) != JSORB_OK || jsorb_set_rectify_maps(ex.handle(), mapx, mapy, w, h, w) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_set_rectify_maps: ") + jsorb_last_error(ex.handle()));
}
inline void ClearRectifyMaps(ORBExtractor &ex)
{
    if (jsorb_clear_rectify_maps(ex.handle()) != JSORB_OK) throw std::runtime_error(std::string("jsorb_clear_rectify_maps: ") + jsorb_last_error(ex.handle()));
}
#ifdef JSORB_WITH_OPENCV
// The two maps exactly as stereo_euroc.cpp:106-107 produces them: CV_32FC1 + CV_32FC1, or (after cv::convertMaps) CV_16SC2 + CV_16UC1.
// (A template over cv::Mat only: its body is checked where it is used, so that headers that declare a reduced cv::Mat still compile.)
template <typename MatT, typename = typename std::enable_if<std::is_same<MatT, cv::Mat>::value>::type>
inline void SetRectifyMaps(ORBExtractor &ex, const MatT &M1, const MatT &M2)
{
    const int k32FC1 = 5, k16SC2 = 11, k16UC1 = 2;      // CV_32FC1, CV_16SC2, CV_16UC1
    const size_t s1 = M1.step[0], s2 = M2.step[0];
    int rc;
    if (M1.rows != M2.rows || M1.cols != M2.cols) throw std::runtime_error("SetRectifyMaps: the two maps differ in size");
    if (M1.type() == k32FC1 && M2.type() == k32FC1 && s1 == s2 && s1 % sizeof(float) == 0)
        rc = jsorb_set_rectify_maps(ex.handle(), reinterpret_cast<const float *>(M1.data), reinterpret_cast<const float *>(M2.data), M1.cols, M1.rows,
                                    (int)(s1 / sizeof(float)));
    else if (M1.type() == k16SC2 && M2.type() == k16UC1 && s1 % 4 == 0 && s2 % 2 == 0)
        rc = jsorb_set_rectify_maps_fixed(ex.handle(), reinterpret_cast<const int16_t *>(M1.data), reinterpret_cast<const uint16_t *>(M2.data), M1.cols,
                                          M1.rows, (int)(s1 / 4), (int)(s2 / 2));
    else
        throw std::runtime_error("SetRectifyMaps: expects CV_32FC1 + CV_32FC1 (same step) or CV_16SC2 + CV_16UC1 maps");
    if (rc != JSORB_OK) throw std::runtime_error(std::string("jsorb_set_rectify_maps: ") + jsorb_last_error(ex.handle()));
}
#endif

// ---- mono / RGB-D Frame (Frame.cpp:251-354, 357-462): the camera, mvKeysUn, the image bounds and the RGB-D depth on the device ----
// Set Tracking's camera ONCE per extractor (Tracking.cpp:80-91); every extract() then also undistorts its keypoints (k_undistort) when k1 != 0.
inline void SetCamera(ORBExtractor &ex, const jsorb_camera &camera)
{
    if (jsorb_set_camera(ex.handle(), &camera) != JSORB_OK) throw std::runtime_error(std::string("jsorb_set_camera: ") + jsorb_last_error(ex.handle()));
}
inline void ClearCamera(ORBExtractor &ex)
{
    if (jsorb_set_camera(ex.handle(), nullptr) != JSORB_OK) throw std::runtime_error(std::string("jsorb_set_camera: ") + jsorb_last_error(ex.handle()));
}

// Frame.cpp:119-196 + UndistortKeyPoints (:718-748): mvKeys, mvKeysUn and the descriptor rows with one synchronisation.
inline void UnpackFrame(ORBExtractor &ex, std::vector<jsorb_keypoint> &mvKeys, std::vector<jsorb_keypoint> &mvKeysUn, std::vector<unsigned char> &descriptors)
{
    const int n = jsorb_n_keypoints(ex.handle(), 0);
    if (n < 0) throw std::runtime_error("UnpackFrame before extract");
    mvKeys.resize(n);
    mvKeysUn.resize(n);
    descriptors.resize((size_t)32 * n);
    if (n && jsorb_unpack_frame_un(ex.handle(), 0, mvKeys.data(), mvKeysUn.data(), descriptors.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_unpack_frame_un: ") + jsorb_last_error(ex.handle()));
}

// Frame::ComputeStereoFromRGBD (Frame.cpp:996-1017) on a raw depth plane - JSORB_DEPTH_U16 (the PNG as read, never converted as a whole) or
// JSORB_DEPTH_F32 - with Tracking's mDepthMapFactor (already inverted, Tracking.cpp:230-234) applied to the sampled pixels only.
inline void ComputeStereoFromRGBD(ORBExtractor &ex, const void *depth, int format, size_t step_bytes, float mDepthMapFactor, float mbf,
                                  std::vector<float> &mvuRight, std::vector<float> &mvDepth)
{
    const int n = jsorb_n_keypoints(ex.handle(), 0);
    if (n < 0) throw std::runtime_error("ComputeStereoFromRGBD before extract");
    mvuRight.assign(n, -1.0f);
    mvDepth.assign(n, -1.0f);
    if (n && jsorb_rgbd_depth(ex.handle(), depth, format, step_bytes, mDepthMapFactor, mbf, mvuRight.data(), mvDepth.data()) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_rgbd_depth: ") + jsorb_last_error(ex.handle()));
}

// Frame::ComputeImageBounds (Frame.cpp:750-778), host only.
inline void ComputeImageBounds(const jsorb_camera &camera, int cols, int rows, float &mnMinX, float &mnMaxX, float &mnMinY, float &mnMaxY)
{
    float b[4];
    if (jsorb_image_bounds(&camera, cols, rows, b) != JSORB_OK) throw std::runtime_error("jsorb_image_bounds: bad camera or image size");
    mnMinX = b[0]; mnMaxX = b[1]; mnMinY = b[2]; mnMaxY = b[3];
}

#ifdef JSORB_WITH_OPENCV
// mvKeys / mvKeysUn as std::vector<cv::KeyPoint> (the memory layout of jsorb_keypoint) and mDescriptors as N x 32 CV_8UC1.
inline void UnpackFrame(ORBExtractor &ex, std::vector<cv::KeyPoint> &mvKeys, std::vector<cv::KeyPoint> &mvKeysUn, cv::Mat &mDescriptors)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(jsorb_keypoint), "jsorb_keypoint mirrors cv::KeyPoint");
    const int n = jsorb_n_keypoints(ex.handle(), 0);
    if (n < 0) throw std::runtime_error("UnpackFrame before extract");
    mvKeys.resize(n);
    mvKeysUn.resize(n);
    mDescriptors = cv::Mat(n, 32, CV_8UC1);
    if (n && jsorb_unpack_frame_un(ex.handle(), 0, reinterpret_cast<jsorb_keypoint *>(mvKeys.data()), reinterpret_cast<jsorb_keypoint *>(mvKeysUn.data()),
                                   mDescriptors.data) != JSORB_OK)
        throw std::runtime_error(std::string("jsorb_unpack_frame_un: ") + jsorb_last_error(ex.handle()));
}

// (Templates over cv::Mat only, like SetRectifyMaps: their bodies are checked where they are used, so that headers that declare a reduced
// cv::Mat still compile.)
// Tracking's mK (3x3 CV_32F) and mDistCoef (4x1 or 5x1 CV_32F), Tracking.cpp:80-91.
template <typename MatT, typename = typename std::enable_if<std::is_same<MatT, cv::Mat>::value>::type>
inline jsorb_camera CameraFromMats(const MatT &mK, const MatT &mDistCoef)
{
    const int k32F = 5;      // CV_32F
    if (mK.type() != k32F || mK.rows != 3 || mK.cols != 3 || mDistCoef.type() != k32F || (mDistCoef.total() != 4 && mDistCoef.total() != 5))
        throw std::runtime_error("camera: expects mK 3x3 CV_32F and mDistCoef with 4 or 5 CV_32F coefficients");
    jsorb_camera c;
    c.fx = mK.template at<float>(0, 0); c.fy = mK.template at<float>(1, 1); c.cx = mK.template at<float>(0, 2); c.cy = mK.template at<float>(1, 2);
    c.k1 = mDistCoef.template at<float>(0); c.k2 = mDistCoef.template at<float>(1);
    c.p1 = mDistCoef.template at<float>(2); c.p2 = mDistCoef.template at<float>(3);
    c.k3 = mDistCoef.total() == 5 ? mDistCoef.template at<float>(4) : 0.0f;
    return c;
}
template <typename MatT, typename = typename std::enable_if<std::is_same<MatT, cv::Mat>::value>::type>
inline void SetCamera(ORBExtractor &ex, const MatT &mK, const MatT &mDistCoef)
{
    SetCamera(ex, CameraFromMats(mK, mDistCoef));
}
template <typename MatT, typename = typename std::enable_if<std::is_same<MatT, cv::Mat>::value>::type>
inline void ComputeImageBounds(const MatT &mK, const MatT &mDistCoef, int cols, int rows, float &mnMinX, float &mnMaxX, float &mnMinY, float &mnMaxY)
{
    ComputeImageBounds(CameraFromMats(mK, mDistCoef), cols, rows, mnMinX, mnMaxX, mnMinY, mnMaxY);
}
// imDepth as Tracking::GrabImageRGBD receives it (CV_16UC1 from the PNG, or CV_32FC1), BEFORE Tracking.cpp:333-334's convertTo: the factor is
// applied to the sampled pixels only.
template <typename MatT, typename = typename std::enable_if<std::is_same<MatT, cv::Mat>::value>::type>
inline void ComputeStereoFromRGBD(ORBExtractor &ex, const MatT &imDepth, float mDepthMapFactor, float mbf, std::vector<float> &mvuRight,
                                  std::vector<float> &mvDepth)
{
    const int k16UC1 = 2, k32FC1 = 5;
    const int format = imDepth.type() == k16UC1 ? JSORB_DEPTH_U16 : imDepth.type() == k32FC1 ? JSORB_DEPTH_F32 : -1;
    if (format < 0) throw std::runtime_error("ComputeStereoFromRGBD: expects a CV_16UC1 or CV_32FC1 depth image");
    ComputeStereoFromRGBD(ex, imDepth.data, format, (size_t)imDepth.step[0], mDepthMapFactor, mbf, mvuRight, mvDepth);
}
#endif

} // namespace Jetson_SLAM

#endif // JSORB_COMPAT_HPP
