// The label selection of PageTextRegionCroppingStep on gfx950 (reference: pipeline/text_detection/
// page_text_region_cropping.py:160-187).
//
// Per attempt the reference asks two STRtrees which label points its window's original_core_box intersects, walks each answer
// in sorted order, and drops a deviate label whose char has no centroid label in the window.  Here every candidate window of a
// page is answered by ONE launch (the pixels are k_crop_planes of crop.hip):
//   k_region_crop_select  one workgroup of 256 lanes per window.  Pass 1 walks the centroid table 256 labels a stride: a lane
//                         tests its label against the closed box (integer compares), sets its char's bit in the window's
//                         preserved-char bitmap and takes its place in the row from a wave64 ballot / popcount prefix, carried
//                         across the waves of the stride through LDS and across strides in a register -- the row comes out in
//                         ascending label order.  Pass 2 walks the deviate table the same way, with the bitmap test added.
//                         The bitmap sits in LDS, sized by the largest char_idx, while that fits 32 KB of bits; otherwise in
//                         a block of the context's scratch per workgroup (as many workgroups as 64 MB of bitmaps allow, at
//                         most 256, then walk the windows), cleared after each window through the kept centroid labels alone.
// The tables are small next to the page (12 bytes a label) and stay in L2 for the windows that follow the first; every value
// is written with plain vector stores, the bitmap bits with vector atomics.
#include "vkx_internal.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int kSelBlock = 256;                  // lanes of a workgroup (four waves)
constexpr int kSelWaves = kSelBlock / 64;
constexpr int kLdsWords = 8192;                 // 32 KB of LDS: char_idx < 262 144
constexpr int kMaxWindows = 4096;
constexpr int kMaxLabels = (1 << 24) - 1;
constexpr int kMaxGlobalGroups = 256;           // workgroups of the scratch-bitmap form ...
constexpr size_t kMaxBitmapBytes = (size_t)64 << 20;   // ... as many as this much scratch holds (2 MB of bits each at most)

// One table of one window: the kept labels' indices into row[0 .. count) in ascending order; -> count (the same in every lane).
// kDeviate: also require the char's bit; else set it.  `carry` are the wave totals of a stride, double-buffered by stride
// parity so that one barrier a stride is enough (a wave reaches the stride after next only behind the barrier of the next).
template <bool kDeviate, bool kLds>
__device__ __forceinline__ int select_table(const int *__restrict__ table, int n, int up, int down, int left, int right,
                                            unsigned *bits, int *__restrict__ row, int (*carry)[kSelWaves])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int kept = 0, parity = 0;
    for (int base = 0; base < n; base += kSelBlock, parity ^= 1) {      // uniform over the workgroup: every lane reaches the barrier
        const int i = base + (int)threadIdx.x;
        bool keep = false;
        if (i < n) {
            const int *rec = table + (size_t)i * 3;
            const int x = rec[0], y = rec[1], c = rec[2];
            keep = left <= x && x <= right && up <= y && y <= down;
            if (keep) {
                unsigned *word = bits + (c >> 5);
                const unsigned bit = 1u << (c & 31);
                if (kDeviate) {
                    // (the scratch form reads past the L1: the bits were set by atomics of other waves, at the L2)
                    const unsigned v = kLds ? *word : __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    keep = (v & bit) != 0;
                } else {
                    atomicOr(word, bit);
                }
            }
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) carry[parity][wave] = __popcll(vote);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kSelWaves; k++) {
            const int c = carry[parity][k];
            before += k < wave ? c : 0;
            total += c;
        }
        if (keep) row[kept + before + __popcll(vote & ((1ull << lane) - 1))] = i;
        kept += total;
    }
    return kept;
}

// grid: one workgroup per window (kLds, `words` of dynamic LDS), or fewer workgroups that walk the windows (scratch bitmaps)
template <bool kLds>
__global__ void __launch_bounds__(kSelBlock) k_region_crop_select(const int4 *__restrict__ windows, int n_windows,
                                                                  const int *__restrict__ centroid, int n_centroid,
                                                                  const int *__restrict__ deviate, int n_deviate, int words,
                                                                  unsigned *__restrict__ scratch, int2 *__restrict__ counts,
                                                                  int *__restrict__ centroid_rows, int *__restrict__ deviate_rows)
{
    __shared__ int carry[2][kSelWaves];
    extern __shared__ unsigned lds_bits[];                              // `words` of them (kLds), none otherwise
    unsigned *bits = kLds ? lds_bits : scratch + (size_t)blockIdx.x * words;
    for (int k = threadIdx.x; k < words; k += kSelBlock) bits[k] = 0;
    __syncthreads();
    for (int win = blockIdx.x; win < n_windows; win += gridDim.x) {
        const int4 box = windows[win];                                   // (up, down, left, right)
        int *crow = centroid_rows + (size_t)win * n_centroid, *drow = deviate_rows + (size_t)win * n_deviate;
        const int nc = select_table<false, kLds>(centroid, n_centroid, box.x, box.y, box.z, box.w, bits, crow, carry);
        __syncthreads();                                                 // every bit of the window is set
        const int nd = nc ? select_table<true, kLds>(deviate, n_deviate, box.x, box.y, box.z, box.w, bits, drow, carry) : 0;
        if (threadIdx.x == 0) counts[win] = make_int2(nc, nd);
        if (!kLds && win + (int)gridDim.x < n_windows) {
            // the next window of this workgroup starts from a clear bitmap: clear the words of the chars kept here
            __syncthreads();                                             // the row is written, the bits are read
            for (int k = threadIdx.x; k < nc; k += kSelBlock)
                __hip_atomic_store(bits + (centroid[(size_t)crow[k] * 3 + 2] >> 5), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
        }
    }
}

}  // namespace

VKX_EXPORT int vkx_region_crop_select_dev(vkx_ctx *ctx, const int32_t *windows_host, int n_windows, const int32_t *centroid_host,
                                          int n_centroid, const int32_t *deviate_host, int n_deviate, int32_t *counts,
                                          int32_t *centroid_rows, int32_t *deviate_rows)
{
    VKX_REQUIRE(n_windows >= 1 && n_windows <= kMaxWindows, "1 .. 4096 windows");
    VKX_REQUIRE(n_centroid >= 0 && n_centroid <= kMaxLabels && n_deviate >= 0 && n_deviate <= kMaxLabels, "0 .. 2^24 - 1 labels");
    VKX_REQUIRE(ctx && windows_host && counts && (centroid_host || n_centroid == 0) && (deviate_host || n_deviate == 0) &&
                    (centroid_rows || n_centroid == 0) && (deviate_rows || n_deviate == 0),
                "NULL argument");
    for (int i = 0; i < n_windows; i++) {
        const int32_t *b = windows_host + (size_t)4 * i;
        VKX_REQUIRE(b[0] <= b[1] && b[2] <= b[3], "a box with down < up or right < left");
    }
    int max_char = -1;
    for (int t = 0; t < 2; t++) {
        const int32_t *table = t ? deviate_host : centroid_host;
        const int n = t ? n_deviate : n_centroid;
        for (int i = 0; i < n; i++) {
            const int c = table[(size_t)3 * i + 2];
            VKX_REQUIRE(c >= 0 && c <= kMaxLabels, "char_idx outside 0 .. 2^24 - 1");
            max_char = std::max(max_char, c);
        }
    }
    const void *outs[3] = {counts, centroid_rows, deviate_rows};
    const size_t bytes[3] = {sizeof(int32_t) * 2 * (size_t)n_windows, sizeof(int32_t) * (size_t)n_windows * n_centroid,
                             sizeof(int32_t) * (size_t)n_windows * n_deviate};
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++)
            VKX_REQUIRE(!vkx_planes_overlap(outs[a], 1, 0, bytes[a], outs[b], 1, 0, bytes[b]), "outputs overlap");

    const int words = (max_char + 32) / 32;                  // 0 without labels
    const bool lds = words <= kLdsWords;
    const int fit = lds ? 0 : (int)std::max<size_t>(1, kMaxBitmapBytes / (sizeof(unsigned) * (size_t)words));
    const int groups = lds ? n_windows : std::min(n_windows, std::min(fit, kMaxGlobalGroups));
    int rc;
    if (!lds && (rc = vkx_scratch_reserve(ctx, &ctx->rc_bitmap, sizeof(unsigned) * (size_t)words * groups))) return rc;
    vkx_tables tab(ctx);
    const size_t win_off = tab.add((size_t)n_windows * 16), cen_off = tab.add((size_t)n_centroid * 12);
    const size_t dev_off = tab.add((size_t)n_deviate * 12);
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<int32_t>(win_off), windows_host, (size_t)n_windows * 16);
    if (n_centroid) memcpy(tab.at<int32_t>(cen_off), centroid_host, (size_t)n_centroid * 12);
    if (n_deviate) memcpy(tab.at<int32_t>(dev_off), deviate_host, (size_t)n_deviate * 12);
    if ((rc = tab.copy_to(&ctx->rc_tables, (size_t)256 << 10))) return rc;      // grows (and syncs) rarely
    char *base = (char *)ctx->rc_tables.ptr;
    {
        VKX_TIMED(ctx, "k_region_crop_select");
        auto kernel = lds ? k_region_crop_select<true> : k_region_crop_select<false>;
        kernel<<<groups, kSelBlock, lds ? sizeof(unsigned) * (size_t)words : 0, ctx->stream>>>((const int4 *)(base + win_off), n_windows, (const int *)(base + cen_off),
                                                      n_centroid, (const int *)(base + dev_off), n_deviate, words,
                                                      (unsigned *)ctx->rc_bitmap.ptr, (int2 *)counts, centroid_rows, deviate_rows);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
