// k_describe.hip - orientation + steered-BRIEF descriptor + output pack, one wave64 (= one workgroup) per keypoint, all
// images of a batch in ONE launch (replaces the reference's 3 kernels x L streams + L device-to-device descriptor copies).
//
// Semantics restated (bit-exact):
//   K8  FASTComputeOrientationGPU  src/cuda/orb_FAST_orientation.cu:17-65  : integer intensity-centroid moments over the
//       r=15 disc (umax table, orb_gpu.cpp:161-182) of the UN-blurred level, angle = atan2f(m01, m10) (libdevice, A.3)
//   K10 ORB_compute_descriptorGPU  src/cuda/orb_descriptor.cu:12-69 : a=cosf, b=sinf (A.4); for pattern point (px,py):
//       row = rint(fma(b,px, a*py)), col = rint(a*px - b*py) (A.5); bit i of byte w = I(p[16w+2i]) < I(p[16w+2i+1])
//       sampled on the 7x7-blurred level (zero outside its ROI)
//   K11 ORB_copy_output_GPU        src/cuda/orb_copy_output.cu:12-45 + D2D copies orb_gpu.cpp:819-831 : SoA pack (A.6)
// MI355X design: both patches are staged in LDS with 16-byte row loads (31 and 37 rows of 48 B loaded from 4-byte aligned columns, 40 B of
// each kept: 1480 B of LDS per keypoint, six workgroups per CU); four consecutive lanes stay inside one row, because the memory pipeline pays per 64-byte chunk a quad of lanes
// touches and the staging is two thirds of this kernel's time.  The 749 disc pixels are summed as dot products of row pairs
// (v_dot4_u32_u8 with multipliers from a 1 KB LDS table) and reduced inside the keypoint's 16 lanes (integer sums are order
// independent); the pattern lives in LDS as FP8 dwords; a wave handles FOUR keypoints (16 lanes each) so that the per-keypoint
// scalar work (atan2f, sinf/cosf, addresses) is issued once per four keypoints; the 256 descriptor bits are produced by 16
// __ballot()s, each delivering 16 bits of each keypoint.
#include "jsorb_launch.h"

#include "describe_tables.h"

namespace jsorb {

#define DESC_R 18          // max |rotated pattern coordinate|: rint(sqrt(338)) = 18
#define BLR_Q 5            // 8-byte units per staged row: 37 px + up to 3 alignment bytes <= 40 (rounds 3-5: 48-byte rows from 8-byte aligned columns)
#define BLR_STRIDE (BLR_Q * 8)
#define KPW 4              // keypoints per wave
#define WPW 4              // waves per workgroup (they share one LDS copy of the pattern)
#define KPWG (KPW * WPW)    // keypoints per workgroup
#define GL (64 / KPW)      // lanes per keypoint
#define PATCH_BYTES (37 * BLR_STRIDE)      // one LDS region per keypoint (1480 B), used first for the un-blurred then for the blurred patch
#ifndef DESC_BLUR_EARLY
#define DESC_BLUR_EARLY 4  // blurred-row loads requested before the un-blurred rows are written to LDS (register budget)
#endif

// the pattern as FP8 dwords and the multipliers of the intensity centroid: describe_tables.h (128-byte aligned: copied into LDS with one
// coalesced load per thread)
__constant__ __align__(128) PatternQ c_pattern_q = make_pattern_q();
__constant__ __align__(128) MomentTab c_moment_tab = make_moment_tab();
#define ORI_LDS_STRIDE 40  // 10 dwords: the 16 rows a keypoint's lanes read at once start 10 banks apart - 16 different (even) banks; four consecutive rows of a store group as well
                           // (rounds 4-5: 14 dwords for the same reason; 12 dwords - 48 bytes - would put them into 8 banks)

// v_writelane_b32 through the LLVM intrinsic (this clang has no __builtin for it; inline asm would hide the VALU-writes-SGPR ->
// v_writelane hazard from the compiler's hazard recognizer)
extern "C" __device__ unsigned writelane_u32(unsigned value, unsigned lane, unsigned old) __asm("llvm.amdgcn.writelane.i32");

// LDS written by some lanes of a wave and read by other lanes of the SAME wave: LDS operations of one wave execute in
// order, so a compiler-level wave barrier (plus wavefront-scope fences) is all the synchronisation needed.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave64 handles KPW keypoints, GL lanes each.  Everything that is identical for all lanes of a keypoint (address set-up,
// atan2f, sinf/cosf, degrees, pack) is thereby issued once per KPW keypoints instead of once per keypoint.  WPW waves form a
// workgroup only to share one LDS copy of the pattern and of the per-level table.  The kernel waits on dependent latencies (every
// pipe is 40-60 % busy), so LDS and registers are kept at what lets 6 workgroups = 24 waves live on a CU (25 984 B, 80 VGPRs).
#ifndef DESC_MIN_WAVES
#define DESC_MIN_WAVES 6      // waves per SIMD the register allocation must allow: 6 workgroups of 4 waves per CU (25 984 B of LDS each) need <= 80 VGPRs
#endif
__global__ __launch_bounds__(64 * WPW, DESC_MIN_WAVES) void k_describe(Geometry g, ImageSrc src, const uint8_t *slab, const uint8_t *blur_slab,
                                                       const unsigned long long *__restrict__ kp, const int *__restrict__ counts,
                                                       float *__restrict__ angles, uint8_t *__restrict__ desc, int32_t *__restrict__ out_kp,
                                                       int n_images, Deliver dl)
{
    __shared__ __align__(16) unsigned char s_patch_all[KPWG][PATCH_BYTES];
    __shared__ __align__(16) unsigned s_pattern[256];
    __shared__ int4 s_level[JSORB_MAX_LEVELS];
    __shared__ __align__(16) unsigned s_moment[8][16][2];
    const int lane = threadIdx.x & 63, wave = uniform_i32(threadIdx.x >> 6);
    const int grp = lane / GL, sl = lane % GL;
    unsigned char *s_patch = s_patch_all[wave * KPW + grp];
    int b, blk;
    if (!xcd_map((g.T + KPWG - 1) / KPWG, n_images, b, blk)) return;
    // the keypoint record is requested together with the keypoint count it will be checked against (slot i_raw < T exists whatever it
    // holds): one memory round trip instead of two in front of the patch loads - the kernel waits on its dependent loads, not on the ALUs
    const int i_raw = blk * KPWG + wave * KPW + grp;
    unsigned long long p = kp[(size_t)b * g.T + min(i_raw, g.T - 1)];
    // what a keypoint needs of its level (pitches, slab offset, scale) goes through a small LDS table filled meanwhile: indexed by the
    // keypoint's level straight from the kernel arguments it was a second, dependent global round trip (and a third for the scale)
    int4 lrec = make_int4(0, 0, 0, 0);
    if (threadIdx.x < (unsigned)g.L) {
        const LevelDesc &l = g.lv[threadIdx.x];
        lrec = make_int4(threadIdx.x == 0 ? src.l0_pitch : l.pitch, (int)l.img_off, l.pitch, __float_as_int(l.scale));
    }
    const unsigned pq = c_pattern_q.v[threadIdx.x];
    uint4 mq = make_uint4(0, 0, 0, 0);
    if (threadIdx.x < 64) mq = reinterpret_cast<const uint4 *>(c_moment_tab.v)[threadIdx.x];
    const int N = uniform_i32(counts[b * (JSORB_MAX_LEVELS + 1) + JSORB_MAX_LEVELS]);
    if (blk * KPWG >= N) return;                      // whole workgroup idle
    static_assert(64 * WPW == 256, "one pattern entry per thread");
    s_pattern[threadIdx.x] = pq;
    if (threadIdx.x < 64) reinterpret_cast<uint4 *>(s_moment)[threadIdx.x] = mq;
    if (threadIdx.x < (unsigned)g.L) s_level[threadIdx.x] = lrec;
    __syncthreads();                                  // the workgroup's pattern copy and level table are complete
    const bool live = i_raw < N;
    const int i = live ? i_raw : N - 1;               // idle groups shadow the last keypoint and write nothing
    if (!live) p = kp[(size_t)b * g.T + i];
    const int lvl = kp_level(p), x = kp_x(p), y = kp_y(p), score = kp_score(p);
    const int4 lv4 = s_level[lvl];
    const int pitch = lv4.x, bpitch = lv4.z;
    const float lv_scale = __int_as_float(lv4.w);
    const uint8_t *img0 = src.l0 + (unsigned long long)b * src.l0_stride;
    const uint8_t *img1 = slab + (unsigned long long)b * g.slab_bytes + (unsigned)lv4.y;
    const uint8_t *img = lvl == 0 ? img0 : img1;
    const uint8_t *bimg = blur_slab + (size_t)b * g.slab_bytes + (unsigned)lv4.y;
    // ---- stage the un-blurred 31-row patch: rows of 3 x 16 B starting at the 4-byte aligned column xa ----
    // The staging is what this kernel's time goes to (two thirds of it), and it is bound by the vector-memory pipeline, which takes
    // the 64 lanes of a load four at a time and pays one L1 access per 64-byte chunk such a quad touches.  So a quad stays inside ONE
    // row: lanes 4q..4q+2 of a keypoint's 16 take the three units of row 4k + q, lane 4q+3 repeats unit 2 (same chunk, no access of
    // its own) and stores nothing.  (Five rows over 15 lanes: every quad straddled two rows, 2.9 accesses per quad instead of 1.6;
    // byte-exact columns with unaligned loads: fewer loads, but each costs 2.2x.)
    // A lane walks down the image with a constant pointer stride and constant LDS offsets.  No bounds tests: a keypoint is >= 20 px
    // from every border, so rows y-15..y+16 exist, xa >= 0, and bytes past the end of a row (the next row or the slab padding) are
    // readable and never used by the disc.
    // Round 6: rows of 40 bytes.  The window of a patch starts at the 4-byte aligned column below its first pixel (31 + 3 resp. 37 + 3 bytes <= 40), so a
    // keypoint's LDS region is 37 x 40 = 1480 bytes instead of 1776 and a workgroup's 25 984 B instead of 30 720: SIX workgroups per CU instead of five -
    // the kernel waits on its loads, resident waves are what it needs (round 5 measured four per CU: -5.5 %).  The 16-byte loads are dword aligned
    // (natural for a dword vector); of a row's three units the third only contributes its first 8 bytes.
    const int xa = (x - JSORB_HALF_PATCH) & ~3, xb = (x - DESC_R) & ~3;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4), aligned(4)));
    const int bq = sl >> 2, bu = min(sl & 3, 2);
    const bool bw = (sl & 3) != 3;
    u32x4 ov[8];
    // Which rows a quad of lanes takes in step k decides the bank conflicts of the LDS stores below (a 16-lane store group is one keypoint's four quads).
    // With the 14-dword rows of rounds 4-5, rows 2 or 4 apart collided two-way and quads 2 / 3 ran one step ahead (docs/HISTORY.md).
    // (10-dword rows: the four consecutive rows 4k .. 4k + 3 of a store group start 10 banks apart and their three units cover 6 + 6 + 6 + 6 different banks -
    // no staggering needed; step 7 holds rows 28 .. 31, of which row 31 is not part of the disc but lies inside the region)
    const int row0 = bq;
    const int row6 = row0 + 24, row7 = row0 + 28;
    {
        const uint8_t *p16 = img + (size_t)(y - JSORB_HALF_PATCH + row0) * pitch + xa + 16 * bu;
        const size_t step = (size_t)4 * pitch;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            ov[k] = *reinterpret_cast<const u32x4 *>(p16);
            p16 += step;
        }
        ov[6] = *reinterpret_cast<const u32x4 *>(img + (size_t)(y - JSORB_HALF_PATCH + row6) * pitch + xa + 16 * bu);
        ov[7] = *reinterpret_cast<const u32x4 *>(img + (size_t)(y - JSORB_HALF_PATCH + row7) * pitch + xa + 16 * bu);
    }
    // the blurred rows (37 x 48 B from column xb) are requested now, into registers, so that their latency hides behind the
    // moments: 4 rows x 3 units of 16 B per step; the last step holds row 36 only - the other quads re-read it and do not write
    u32x4 bl[10];
    const uint8_t *pb16 = bimg + (size_t)(y - DESC_R + bq) * bpitch + xb + 16 * bu;
    const size_t bstep = (size_t)4 * bpitch;
#pragma unroll
    for (int k = 0; k < DESC_BLUR_EARLY; k++) {
        bl[k] = *reinterpret_cast<const u32x4 *>(pb16);
        pb16 += bstep;
    }
    if (bw) {
        uint2 *const od = reinterpret_cast<uint2 *>(s_patch + row0 * ORI_LDS_STRIDE + 16 * bu);
        const bool second = bu < 2;                     // 40-byte rows: the third unit's upper 8 bytes lie beyond the row
#pragma unroll
        for (int k = 0; k < 6; k++) {
            od[k * (4 * ORI_LDS_STRIDE / 8)] = make_uint2(ov[k].x, ov[k].y);
            if (second) od[k * (4 * ORI_LDS_STRIDE / 8) + 1] = make_uint2(ov[k].z, ov[k].w);
        }
        uint2 *const o6 = reinterpret_cast<uint2 *>(s_patch + row6 * ORI_LDS_STRIDE + 16 * bu);
        o6[0] = make_uint2(ov[6].x, ov[6].y);
        if (second) o6[1] = make_uint2(ov[6].z, ov[6].w);
        uint2 *const o7 = reinterpret_cast<uint2 *>(s_patch + row7 * ORI_LDS_STRIDE + 16 * bu);
        o7[0] = make_uint2(ov[7].x, ov[7].y);
        if (second) o7[1] = make_uint2(ov[7].z, ov[7].w);
    }
    // (the rest of the blurred rows once the registers of the un-blurred ones are free: 6 waves per SIMD need <= 80 VGPRs)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = DESC_BLUR_EARLY; k < 9; k++) {
        bl[k] = *reinterpret_cast<const u32x4 *>(pb16);
        pb16 += bstep;
    }
    bl[9] = *reinterpret_cast<const u32x4 *>(bimg + (size_t)(y - DESC_R + 36) * bpitch + xb + 16 * bu);
    wave_lds_sync();

    // ---- intensity centroid over the disc (see MomentTab) ----
    int m10, m01;
    {
        const unsigned al = (unsigned)(x - JSORB_HALF_PATCH) & 3u, sh = al;      // (the window starts at most 3 bytes below the patch)
        const unsigned *r1 = reinterpret_cast<const unsigned *>(s_patch + (JSORB_HALF_PATCH + sl) * ORI_LDS_STRIDE);
        const unsigned *r2 = reinterpret_cast<const unsigned *>(s_patch + (JSORB_HALF_PATCH - sl) * ORI_LDS_STRIDE);
        unsigned p1 = 0, p2 = 0, n1 = 0, n2 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const uint2 t = reinterpret_cast<const uint2 *>(s_moment)[d * 16 + sl];
            const unsigned w1 = __builtin_amdgcn_alignbyte(r1[d + 1], r1[d], sh);
            const unsigned w2 = __builtin_amdgcn_alignbyte(r2[d + 1], r2[d], sh);
            if (d < 4) {
                n1 = __builtin_amdgcn_udot4(w1, t.x, n1, false);
                n2 = __builtin_amdgcn_udot4(w2, t.x, n2, false);
            } else {
                p1 = __builtin_amdgcn_udot4(w1, t.x, p1, false);
                p2 = __builtin_amdgcn_udot4(w2, t.x, p2, false);
            }
            s1 = __builtin_amdgcn_udot4(w1, t.y, s1, false);
            s2 = __builtin_amdgcn_udot4(w2, t.y, s2, false);
        }
        m10 = (int)(p1 - n1) + (sl ? (int)(p2 - n2) : 0);      // lane 0: both rows are row y
        m01 = sl * (int)(s1 - s2);
    }
    static_assert(GL == 16, "the lane group of a keypoint is one DPP row");
    m10 = row16_sum_i32(m10);                         // reduce inside the keypoint's lane group
    m01 = row16_sum_i32(m01);
    const float angle = atan2f_ref(m01, m10);
    const float a = sincos_core_ref(angle, 1), bs = sincos_core_ref(angle, 0);

    // ---- the blurred patch replaces the un-blurred one in LDS ----
    wave_lds_sync();
    if (bw) {
        // 40-byte rows are 8-byte aligned: two 8-byte stores per unit, the third unit's second one dropped
        uint2 *const dst = reinterpret_cast<uint2 *>(s_patch + bq * BLR_STRIDE + 16 * bu);
        const bool second = bu < 2;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            dst[k * (4 * BLR_STRIDE / 8)] = make_uint2(bl[k].x, bl[k].y);
            if (second) dst[k * (4 * BLR_STRIDE / 8) + 1] = make_uint2(bl[k].z, bl[k].w);
        }
        if (bq == 0) {
            dst[9 * (4 * BLR_STRIDE / 8)] = make_uint2(bl[9].x, bl[9].y);
            if (second) dst[9 * (4 * BLR_STRIDE / 8) + 1] = make_uint2(bl[9].z, bl[9].w);
        }
    }
    wave_lds_sync();

    // ---- steered BRIEF: 256 / GL steps, every step one __ballot() = GL descriptor bits of each of the KPW keypoints ----
    // Both points of a bit go through the packed-f32 pipe together (7 packed instructions for 2 rows + 2 columns):
    //   row = fma(b, px, a*py), col = a*px - b*py  (A.5; (-b)*py = -(b*py) exactly, so a*px + (-b)*py is the same subtraction)
    // rint() by the magic-number addition (round-to-nearest-even float add, |value| <= 18): as_int(v + 1.5*2^23) = 0x4B400000 + rint(v).
    // The column's magic number also carries the EVEN part of the keypoint's LDS byte address (patch base + 18 rows + x - xb): the sum
    // stays inside [2^23, 2^24), where floats are the integers, and an even offset keeps the tie-to-even choice of rint() unchanged.
    // v_mad_u32_u24 takes the low 24 bits of the row word (0x400000 + row) times the row stride plus the column word; one integer
    // add removes the magic numbers (and restores the odd bit): 2 integer instructions per point.
    typedef float f2 __attribute__((ext_vector_type(2)));
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)s_patch;
    const unsigned kaddr = lds_base + (unsigned)(DESC_R * BLR_STRIDE + (x - xb));
    const float col_magic = 12582912.0f + (float)(kaddr & ~1u);
    const unsigned kfix = (kaddr & 1u) - 0x400000u * BLR_STRIDE - 0x4B400000u;
    const f2 a2 = (f2){a, a}, b2 = (f2){bs, bs}, nb2 = (f2){-bs, -bs}, rmagic2 = (f2){12582912.0f, 12582912.0f}, cmagic2 = (f2){col_magic, col_magic};
    uint4 pc[4];
#pragma unroll
    for (int c = 0; c < 4; c++) pc[c] = reinterpret_cast<const uint4 *>(s_pattern)[sl * 4 + ((c + (sl >> 2)) & 3)];
    // step it delivers, through one __ballot (= the v_cmp itself), bit sl of descriptor word it of each of the 4 keypoints.  The
    // 16 ballots are parked in lanes 0..15 of two VGPRs (v_writelane), so that at the end lane (grp, sl) fetches ballot sl with
    // one shuffle and keeps its keypoint's 16 bits - instead of a 16-way select per lane.
    // (Round 6: the point reads of step it + 1 / it + 2 requested before the comparison of step it waits for its own - s_waitcnt lgkmcnt(2) / (4) instead of (0),
    // 80 VGPRs either way: +-0 in two A/B runs, the other waves of the SIMD already cover that round trip; profiles/r06_experiments.txt section 27.)
    unsigned blo = 0, bhi = 0;
#pragma unroll
    for (int it = 0; it < 256 / GL; it++) {
        const uint4 pc4 = pc[it >> 2];
        const int pw = (int)((it & 3) == 0 ? pc4.x : (it & 3) == 1 ? pc4.y : (it & 3) == 2 ? pc4.z : pc4.w);      // x0 x1 y0 y1 of descriptor bit it*GL + sl
        const f2 X = __builtin_amdgcn_cvt_pk_f32_fp8(pw, false), Y = __builtin_amdgcn_cvt_pk_f32_fp8(pw, true);
        const f2 rowf = __builtin_elementwise_fma(b2, X, a2 * Y) + rmagic2;
        const f2 colf = (a2 * X + nb2 * Y) + cmagic2;
        const unsigned o0 = __umul24(__float_as_uint(rowf.x), BLR_STRIDE) + __float_as_uint(colf.x) + kfix;
        const unsigned o1 = __umul24(__float_as_uint(rowf.y), BLR_STRIDE) + __float_as_uint(colf.y) + kfix;
        const int t0 = *(const __attribute__((address_space(3))) unsigned char *)(uintptr_t)o0;
        const int t1 = *(const __attribute__((address_space(3))) unsigned char *)(uintptr_t)o1;
        const unsigned long long bits = __ballot(t0 < t1);
        blo = writelane_u32((unsigned)bits, it, blo);
        bhi = writelane_u32((unsigned)(bits >> 32), it, bhi);
    }
    const unsigned w_lo = (unsigned)__shfl((int)blo, sl, 64), w_hi = (unsigned)__shfl((int)bhi, sl, 64);
    const unsigned mychunk = ((grp & 2) ? w_hi : w_lo) >> (16 * (grp & 1));      // stored as 16 bits below
    if (live) {
        static_assert(GL == 16, "descriptor store below assumes 16 lanes x 16 bits");
        reinterpret_cast<unsigned short *>(desc + ((size_t)b * g.T + i) * 32)[sl] = (unsigned short)mychunk;
        // single-image calls: the same bytes also go to the caller's device buffer and to the pinned host mirror (struct Deliver)
        if (dl.desc_dev) reinterpret_cast<unsigned short *>(dl.desc_dev + (size_t)i * 32)[sl] = (unsigned short)mychunk;
        if (dl.desc_host) reinterpret_cast<unsigned short *>(dl.desc_host + (size_t)i * 32)[sl] = (unsigned short)mychunk;
        // ---- SoA pack: lanes 0..5 of the group write the six blocks (x, y, score, angle in degrees, octave, size) ----
        if (sl < 6) {
            const float xy = (float)(sl == 0 ? x : y) * lv_scale;
            int val = (int)xy;
            val = sl == 2 ? score : val;
            val = sl == 3 ? (int)__float_as_uint((float)((double)angle * 57.29577951308232)) : val;
            val = sl == 4 ? lvl : val;
            val = sl == 5 ? (int)(lv_scale * 31.0f) : val;
            out_kp[(size_t)b * 6 * g.T + (unsigned)(sl * N + i)] = val;
            if (dl.kp_dev) dl.kp_dev[(unsigned)(sl * N + i)] = val;
            if (dl.kp_host) dl.kp_host[(unsigned)(sl * N + i)] = val;
        }
        if (sl == 6) angles[(size_t)b * g.T + i] = angle;
    }
}

// for the single-frame graph of jsorb_extract.hip: which node of a captured frame is this kernel, and which of its arguments is `dl`
const void *describe_kernel_address() { return reinterpret_cast<const void *>(&k_describe); }
int describe_kernel_deliver_arg() { return 10; }

void launch_describe(const Geometry &g, const ImageSrc &src, const uint8_t *slab, const uint8_t *blur_slab,
                     const unsigned long long *kp, const int *counts, float *angles, uint8_t *desc, int32_t *out_kp,
                     int n_images, hipStream_t s, Deliver dl)
{
    hipLaunchKernelGGL(k_describe, xcd_grid((g.T + KPWG - 1) / KPWG, n_images), dim3(64 * WPW), 0, s, g, src, slab, blur_slab, kp, counts,
                       angles, desc, out_kp, n_images, dl);
}

} // namespace jsorb
