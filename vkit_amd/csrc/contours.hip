// Mask.to_disconnected_polygons on gfx950 (reference: element/mask.py:657-733): cv.findContours(mask * 255, RETR_TREE, method)
// filtered to the contours whose hierarchy parent is -1, for a batch of masks, restated from the published algorithm
// (Suzuki & Abe 1985, the trace of OpenCV's icvFetchContour; tests/contours_restate.py is the numpy restatement).
//
// Which borders: foreground (> 0) is 8-connected, background 4-connected, the plane is surrounded by background.  A foreground
// component is kept when the background pixel west of its raster-first pixel lies outside the plane or belongs to the background
// region that reaches the plane's edge; kept components are ordered by that pixel.  EIGHT launches whatever the number of masks,
// components and points, no host-side loop, no synchronisation:
//   k_contour_label_tiles   one lane a pixel, one workgroup a 32 x 8 tile of one mask: union-find in LDS over the pixel's earlier
//                           neighbours of its own class (W N NW NE for foreground, W N for background), the smaller index the
//                           root; the tile's labels go to the mask's label plane as node = 1 + y * w + x (node 0 is the frame).
//   k_contour_merge         the lanes on a tile's first row, first column and last column unite across the seam on the global
//                           plane (atomic-min unions); background on the plane's edge unites with node 0.  A component's root is
//                           now its raster-first pixel, and a background region reaches the edge iff its root is node 0.
//   k_contour_flags         one wave per 64 pixels in raster order: a lane whose pixel is a foreground root applies the start
//                           test (a find from its west neighbour -- the flatten, limited to the pixels the test reads); the
//                           wave's ballot is one word of the mask's start bitmap.
//   k_contour_compact       one workgroup a mask: popcount, scan, write -- the starts of the mask in raster order.
//   k_contour_mask_scan     one workgroup: the first contour of every mask.
//   k_contour_trace<false>  one wave a kept component: the 64 lanes read an 8 x 8 window around the current pixel, one ballot
//                           makes it a 64-bit map in every lane, and the trace walks inside it -- the eight neighbours are bit
//                           picks, the search for the next direction a rotate and a find-first-set that every lane does alike
//                           -- until it leaves the window's inner 6 x 6: one memory round trip for up to six steps instead of up
//                           to eight a step.  Counts the contour's points.
//   k_contour_offsets       one workgroup: the scan of the lengths, totals, the capacity decision, n_contours / status / lengths /
//                           offsets.
//   k_contour_trace<true>   the same trace, writing points; skipped as a whole when a capacity is short, and bounded by the
//                           counted length: nothing partial, nothing out of bounds.
// Every trace loop is capped at 8 * h * w + 8 steps (a border visits a (pixel, direction) pair once); a wave that reaches the cap,
// or stands on a pixel without neighbours mid-trace (a plane that changed under it), gives up and marks its mask's status.
// Plain vector stores and vector atomics only.
#include "vkx_internal.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int kTW = 32, kTH = 8;                 // the labelling tile: one workgroup of 256 lanes
constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;                 // the single-workgroup scans
constexpr int kMaxMasks = 4096;
constexpr int kMaxSide = 32767;
constexpr long long kMaxPixels = 2147483640ll;   // 2^31 - 8: node numbers fit int32
constexpr long long kMaxBatchPixels = 1ll << 32; // 16 GB of labels: every tile, word and start count of a batch fits int32
constexpr int kMaxTraceGroups = 4096;            // workgroups of four waves that stride over the kept components

struct Rec {
    const uint8_t *src;
    long long step;
    long long lab_off;                           // node 0 of the mask in the label plane
    int h, w;
    int tile_start, word_start, start_base, start_room;  // the mask's starts: ceil(h / 2) * ceil(w / 2) slots from start_base
};

template <int kScope>
__device__ __forceinline__ int uf_find(int *L, int a)
{
    for (;;) {
        const int p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, kScope);
        if (p == a) return a;
        a = p;                                   // parents only decrease: the walk ends
    }
}
// Lock-free union by index: the larger root hangs under the smaller one.  A root that stopped being one under our hands (the
// atomic-min returns what it held) hands us its new parent to go on from.
template <int kScope>
__device__ __forceinline__ void uf_union(int *L, int a, int b)
{
    for (;;) {
        a = uf_find<kScope>(L, a);
        b = uf_find<kScope>(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, kScope);
        if (old == b) return;
        b = old;
    }
}

// grid: every 32 x 8 tile of every mask
__global__ void __launch_bounds__(kBlock) k_contour_label_tiles(const Rec *__restrict__ recs, int n, int *__restrict__ labels)
{
    __shared__ int lab[kBlock];
    __shared__ unsigned char cls[kBlock];
    int rx, ry;
    const int g = vkd::box_tile_pixel<kTW, kTH>(n, [&](int i) { return recs[i].tile_start; }, [&](int i) { return recs[i].w; }, rx, ry);
    const Rec r = recs[g];
    const int t = threadIdx.x, tx = t & (kTW - 1), ty = t / kTW;
    const bool inside = rx < r.w && ry < r.h;
    const int v = inside ? (r.src[(ptrdiff_t)ry * r.step + rx] > 0 ? 1 : 0) : 2;      // 2: outside the plane, unites with nothing
    cls[t] = (unsigned char)v;
    lab[t] = t;
    __syncthreads();
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    if (inside) {
        if (tx > 0 && cls[t - 1] == v) uf_union<WG>(lab, t, t - 1);
        if (ty > 0 && cls[t - kTW] == v) uf_union<WG>(lab, t, t - kTW);
        if (v == 1 && ty > 0) {
            if (tx > 0 && cls[t - kTW - 1] == 1) uf_union<WG>(lab, t, t - kTW - 1);
            if (tx < kTW - 1 && cls[t - kTW + 1] == 1) uf_union<WG>(lab, t, t - kTW + 1);
        }
    }
    __syncthreads();
    if (inside) {
        const int root = uf_find<WG>(lab, t);
        int *L = labels + r.lab_off;
        L[1 + ry * r.w + rx] = 1 + (ry - ty + root / kTW) * r.w + (rx - tx + (root & (kTW - 1)));
        if (rx == 0 && ry == 0) L[0] = 0;
    }
}

// grid: as k_contour_label_tiles
__global__ void __launch_bounds__(kBlock) k_contour_merge(const Rec *__restrict__ recs, int n, int *__restrict__ labels)
{
    int rx, ry;
    const int g = vkd::box_tile_pixel<kTW, kTH>(n, [&](int i) { return recs[i].tile_start; }, [&](int i) { return recs[i].w; }, rx, ry);
    const Rec r = recs[g];
    const int t = threadIdx.x, tx = t & (kTW - 1), ty = t / kTW;
    if (rx >= r.w || ry >= r.h) return;
    const bool plane_edge = rx == 0 || ry == 0 || rx == r.w - 1 || ry == r.h - 1;
    if (!(tx == 0 || ty == 0 || tx == kTW - 1 || plane_edge)) return;
    constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
    const bool v = r.src[(ptrdiff_t)ry * r.step + rx] > 0;
    int *L = labels + r.lab_off;
    const int node = 1 + ry * r.w + rx;
    auto across = [&](int dx, int dy) {                       // an earlier neighbour of the same class in another tile
        const int x = rx + dx, y = ry + dy;
        if ((unsigned)(tx + dx) < (unsigned)kTW && ty + dy >= 0) return;
        if ((unsigned)x >= (unsigned)r.w || y < 0) return;
        if ((r.src[(ptrdiff_t)y * r.step + x] > 0) == v) uf_union<DEV>(L, node, 1 + y * r.w + x);
    };
    across(-1, 0);
    across(0, -1);
    if (v) {
        across(-1, -1);
        across(1, -1);
    } else if (plane_edge) {
        uf_union<DEV>(L, node, 0);
    }
}

// grid: four waves a workgroup, one wave per 64 pixels (raster order) of every mask
__global__ void __launch_bounds__(kBlock) k_contour_flags(const Rec *__restrict__ recs, int n, int total_words, int *__restrict__ labels,
                                                           unsigned long long *__restrict__ words)
{
    const int kw = blockIdx.x * (kBlock / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (kw >= total_words) return;                            // the whole wave
    const int g = vkd::last_at_most(n, kw, [&](int i) { return recs[i].word_start; });
    const Rec r = recs[g];
    const long long i = (long long)(kw - r.word_start) * 64 + lane;
    bool start = false;
    if (i < (long long)r.h * r.w) {
        const int x = (int)(i % r.w), y = (int)(i / r.w);
        if (r.src[(ptrdiff_t)y * r.step + x] > 0) {
            int *L = labels + r.lab_off;
            const int node = (int)i + 1;
            // a foreground root is the raster-first pixel of its component: its west neighbour, if any, is background
            if (L[node] == node) start = x == 0 || uf_find<__HIP_MEMORY_SCOPE_AGENT>(L, node - 1) == 0;
        }
    }
    const unsigned long long vote = __ballot(start);
    if (lane == 0) words[kw] = vote;
}

// The exclusive prefix of v over the workgroup (NT lanes) and its total; two barriers.
template <int NT>
__device__ __forceinline__ long long block_scan_excl(long long v, long long *wave_total, long long &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    __syncthreads();                                          // the totals of the call before are read
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) {
        const long long c = wave_total[k];
        before += k < wave ? c : 0;
        total += c;
    }
    return before + incl - v;
}

// grid: one workgroup a mask
__global__ void __launch_bounds__(kBlock) k_contour_compact(const Rec *__restrict__ recs, const unsigned long long *__restrict__ words,
                                                             int *__restrict__ starts, int *__restrict__ n_starts)
{
    __shared__ long long wave_total[kBlock / 64];
    const Rec r = recs[blockIdx.x];
    const int nw = (int)(((long long)r.h * r.w + 63) >> 6);
    long long kept = 0;
    for (int k0 = 0; k0 < nw; k0 += kBlock) {                 // uniform over the workgroup
        const int k = k0 + (int)threadIdx.x;
        unsigned long long bits = k < nw ? words[r.word_start + k] : 0ull;
        long long total;
        long long pos = kept + block_scan_excl<kBlock>(__popcll(bits), wave_total, total);
        while (bits) {
            if (pos < r.start_room) starts[r.start_base + pos] = k * 64 + (__ffsll((long long)bits) - 1);
            pos++;
            bits &= bits - 1;
        }
        kept += total;
    }
    if (threadIdx.x == 0) n_starts[blockIdx.x] = (int)std::min<long long>(kept, r.start_room);      // (never more: one component a 2 x 2 block)
}

// grid: one workgroup.  first[m]: the first contour of mask m among all contours, first[n] their number.
__global__ void __launch_bounds__(kScanBlock) k_contour_mask_scan(int n, const int *__restrict__ n_starts, int *__restrict__ first,
                                                                   int *__restrict__ hit)
{
    __shared__ long long wave_total[kScanBlock / 64];
    long long carry = 0;
    for (int base = 0; base < n; base += kScanBlock) {
        const int m = base + (int)threadIdx.x;
        long long total;
        const long long before = block_scan_excl<kScanBlock>(m < n ? n_starts[m] : 0, wave_total, total);
        if (m < n) {
            first[m] = (int)(carry + before);
            hit[m] = 0;
        }
        carry += total;
    }
    if (threadIdx.x == 0) first[n] = (int)carry;
}

__device__ __forceinline__ int dir_dx(int s) { return (int)((0x901Au >> (2 * s)) & 3u) - 1; }   // E NE N NW W SW S SE: 1 1 0 -1 -1 -1 0 1
__device__ __forceinline__ int dir_dy(int s) { return (int)((0xA901u >> (2 * s)) & 3u) - 1; }   //                      0 -1 -1 -1 0 1 1 1

// (what a wave knows to be the same in all its lanes, said to the compiler: the trace then runs on the scalar unit)
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long wave_uniform(long long v)
{
    return (long long)(((unsigned long long)(unsigned)wave_uniform((int)(v >> 32)) << 32) | (unsigned)wave_uniform((int)v));
}

// grid: workgroups of four waves striding over the kept components; a wave traces one component at a time
template <bool kWrite>
__global__ void __launch_bounds__(kBlock) k_contour_trace(const Rec *__restrict__ recs, int n, int method, const int *__restrict__ first,
                                                           const int *__restrict__ starts, long long *__restrict__ lens,
                                                           const long long *__restrict__ offs, int *__restrict__ hit,
                                                           const int *__restrict__ fit, int2 *__restrict__ points)
{
    const int lane = threadIdx.x & 63, total = first[n];
    if (kWrite && !*fit) return;
    for (int c = blockIdx.x * (kBlock / 64) + wave_uniform((int)(threadIdx.x >> 6)); c < total; c += gridDim.x * (kBlock / 64)) {
        const int m = vkd::last_at_most(n, c, [&](int i) { return first[i]; });
        const Rec r = recs[m];
        const int i0 = wave_uniform(starts[r.start_base + (c - first[m])]);
        const int x0 = i0 % r.w, y0 = i0 / r.w;
        const long long room = kWrite ? wave_uniform(lens[c]) : 0, out = kWrite ? wave_uniform(offs[c]) : 0;
        // The wave holds an 8 x 8 window of the plane as one ballot, a lane a pixel.  around(x, y, s): the eight neighbours of
        // (x, y) as a byte, bit k the neighbour in direction k, the same in every lane; s is the direction the trace came by.
        // When (x, y) leaves the window's inner 6 x 6 the window is read again with the pixel one in from the side it entered
        // through: a straight run takes six steps a memory round trip.
        int wx0 = INT_MIN / 2, wy0 = INT_MIN / 2;
        unsigned long long window = 0;
        auto around = [&](int x, int y, int s) {
            if (x - 1 < wx0 || x + 1 > wx0 + 7 || y - 1 < wy0 || y + 1 > wy0 + 7) {       // uniform over the wave
                const int dx = dir_dx(s), dy = dir_dy(s);
                wx0 = x - (dx > 0 ? 1 : dx < 0 ? 6 : 3);
                wy0 = y - (dy > 0 ? 1 : dy < 0 ? 6 : 3);
                const int px = wx0 + (lane & 7), py = wy0 + (lane >> 3);
                window = __ballot((unsigned)px < (unsigned)r.w && (unsigned)py < (unsigned)r.h && r.src[(ptrdiff_t)py * r.step + px] > 0);
            }
            // the 3 x 3 block around the pixel (1 .. 6 in the window): rows `up`, `mid`, `down`, bit 0 the west column
            const unsigned block = (unsigned)(window >> ((y - wy0 - 1) * 8 + (x - wx0 - 1)));
            const unsigned up = block & 7u, mid = (block >> 8) & 7u, down = (block >> 16) & 7u;
            // E | NE N NW (the upper row from east to west: its three bits reversed) | W | SW S SE
            return (mid >> 2) | ((__brev(up) >> 29) << 1) | ((mid & 1u) << 4) | (down << 5);
        };
        auto emit = [&](long long k, int x, int y) {
            if (kWrite && lane == 0 && k < room) points[out + k] = make_int2(x, y);
        };
        unsigned nb = around(x0, y0, 7);                      // the first pixel of a component: all of it lies east and south
        long long len = 0;
        int s = 4;
        bool found = false;
        for (int k = 0; k < 7 && !found; k++) {               // 3 2 1 0 7 6 5: clockwise from the west
            s = (s - 1) & 7;
            found = (nb >> s) & 1u;
        }
        if (!found) {
            emit(0, x0, y0);
            len = 1;
        } else {
            const int x1 = x0 + dir_dx(s), y1 = y0 + dir_dy(s);
            int x3 = x0, y3 = y0, prev_s = s ^ 4;
            const long long cap = 8ll * r.h * r.w + 8;
            bool gave_up = false;
            for (long long step = 0;; step++) {
                if (step >= cap || nb == 0) { gave_up = true; break; }
                const int from = (s + 1) & 7;                  // counter-clockwise from the direction after s
                const unsigned turned = ((nb >> from) | (nb << (8 - from))) & 0xffu;
                s = (from + __ffs((int)turned) - 1) & 7;
                const int x4 = x3 + dir_dx(s), y4 = y3 + dir_dy(s);
                if (method == 1 || s != prev_s) {
                    emit(len, x3, y3);
                    len++;
                    prev_s = s;
                }
                if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
                x3 = x4;
                y3 = y4;
                nb = around(x3, y3, s);
                s = (s + 4) & 7;
            }
            if (gave_up) {
                len = 0;
                if (lane == 0) atomicOr(hit + m, 1);
            }
        }
        if (!kWrite && lane == 0) lens[c] = len;
    }
}

// grid: one workgroup
__global__ void __launch_bounds__(kScanBlock) k_contour_offsets(int n, const int *__restrict__ first, const long long *__restrict__ lens,
                                                                 long long *__restrict__ offs, const int *__restrict__ hit,
                                                                 int cap_contours, int cap_points, int *__restrict__ fit_flag,
                                                                 int *__restrict__ n_contours, int *__restrict__ contour_len,
                                                                 int *__restrict__ contour_off, long long *__restrict__ totals,
                                                                 int *__restrict__ status)
{
    __shared__ long long wave_total[kScanBlock / 64];
    const int total = first[n];
    long long n_points = 0;
    for (int base = 0; base < total; base += kScanBlock) {
        const int c = base + (int)threadIdx.x;
        long long sum;
        const long long before = block_scan_excl<kScanBlock>(c < total ? lens[c] : 0, wave_total, sum);
        if (c < total) offs[c] = n_points + before;
        n_points += sum;
    }
    __syncthreads();                                          // offs of the whole batch, written by this workgroup
    const bool fit = total <= cap_contours && n_points <= cap_points;
    for (int m = threadIdx.x; m < n; m += kScanBlock) {
        const int c0 = first[m], c1 = first[m + 1];
        const long long p0 = c0 < total ? offs[c0] : n_points, p1 = c1 < total ? offs[c1] : n_points;
        totals[2 * m] = c1 - c0;
        totals[2 * m + 1] = p1 - p0;
        n_contours[m] = fit ? c1 - c0 : 0;
        status[m] = (fit ? 0 : VKX_CONTOURS_SHORT) | (hit[m] ? VKX_CONTOURS_GAVE_UP : 0);
    }
    if (fit)
        for (int c = threadIdx.x; c < total; c += kScanBlock) {
            contour_len[c] = (int)lens[c];
            contour_off[c] = (int)offs[c];
        }
    if (threadIdx.x == 0) *fit_flag = fit;
}

}  // namespace

VKX_EXPORT int vkx_mask_contours_dev(vkx_ctx *ctx, const vkx_contour_mask *masks_host, int n_masks, int method, int cap_contours,
                                     int cap_points, int32_t *n_contours, int32_t *contour_len, int32_t *contour_off, int32_t *points,
                                     int64_t *totals, int32_t *status)
{
    VKX_REQUIRE(n_masks >= 1 && n_masks <= kMaxMasks, "1 .. 4096 masks");
    VKX_REQUIRE(ctx && masks_host && n_contours && contour_len && contour_off && points && totals && status, "NULL argument");
    VKX_REQUIRE(method == VKX_CHAIN_APPROX_NONE || method == VKX_CHAIN_APPROX_SIMPLE, "method is neither CHAIN_APPROX_NONE (1) nor CHAIN_APPROX_SIMPLE (2)");
    VKX_REQUIRE(cap_contours >= 0 && cap_points >= 0, "a negative capacity");
    const vkx_plane_bytes outs[6] = {{n_contours, sizeof(int32_t) * (size_t)n_masks},   {contour_len, sizeof(int32_t) * (size_t)cap_contours},
                                     {contour_off, sizeof(int32_t) * (size_t)cap_contours}, {points, sizeof(int32_t) * 2 * (size_t)cap_points},
                                     {totals, sizeof(int64_t) * 2 * (size_t)n_masks},   {status, sizeof(int32_t) * (size_t)n_masks}};
    VKX_REQUIRE(vkx_planes_disjoint(outs, 6), "outputs overlap one another");
    std::vector<Rec> recs((size_t)n_masks);
    long long labels = 0, tiles = 0, words = 0, bound = 0, pixels = 0;
    for (int i = 0; i < n_masks; i++) {
        const vkx_contour_mask &k = masks_host[i];
        VKX_REQUIRE(k.mask, "NULL argument");
        VKX_REQUIRE(k.h >= 1 && k.h <= kMaxSide && k.w >= 1 && k.w <= kMaxSide, "a mask side outside 1 .. 32767");
        const long long area = (long long)k.h * k.w;
        VKX_REQUIRE(area <= kMaxPixels, "a mask of more than 2^31 - 8 pixels");
        VKX_REQUIRE_PITCH(k.step, k.w, k.h);
        for (const vkx_plane_bytes &o : outs)
            VKX_REQUIRE(!vkx_planes_overlap(k.mask, k.h, (ptrdiff_t)k.step, (size_t)k.w, o.ptr, 1, 0, o.bytes), "an output overlaps a mask");
        const long long room = (long long)((k.h + 1) / 2) * ((k.w + 1) / 2);      // 8-connected components of an h x w plane: one a 2 x 2 block at most
        recs[i] = Rec{k.mask, (long long)k.step, labels, k.h, k.w, (int)tiles, (int)words, (int)bound, (int)room};
        labels += area + 1;
        tiles += (long long)((k.w + kTW - 1) / kTW) * ((k.h + kTH - 1) / kTH);
        words += (area + 63) >> 6;
        bound += room;
        pixels += area;
        VKX_REQUIRE(pixels <= kMaxBatchPixels, "a batch of more than 2^32 pixels");
    }

    // the planes of the call in ONE scratch block: labels | start bitmaps | starts | lengths | offsets | per-mask counters | the flag
    size_t bytes = 0;
    auto part = [&](size_t n) { const size_t off = vkx_align256(bytes); bytes = off + n; return off; };
    const size_t lab_off = part(sizeof(int) * (size_t)labels), word_off = part(sizeof(unsigned long long) * (size_t)words);
    const size_t start_off = part(sizeof(int) * (size_t)bound), len_off = part(sizeof(long long) * (size_t)bound);
    const size_t off_off = part(sizeof(long long) * (size_t)bound), count_off = part(sizeof(int) * (size_t)n_masks);
    const size_t first_off = part(sizeof(int) * ((size_t)n_masks + 1)), hit_off = part(sizeof(int) * (size_t)n_masks);
    const size_t fit_off = part(sizeof(int));
    int rc;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->contour_planes, bytes))) return rc;
    vkx_tables tab(ctx);
    if ((rc = tab.take(sizeof(Rec) * recs.size()))) return rc;
    memcpy(tab.at<Rec>(0), recs.data(), sizeof(Rec) * recs.size());
    if ((rc = tab.copy_to(&ctx->contour_tables, (size_t)64 << 10))) return rc;      // grows (and syncs) rarely
    const Rec *d_recs = (const Rec *)ctx->contour_tables.ptr;
    char *base = (char *)ctx->contour_planes.ptr;
    int *d_labels = (int *)(base + lab_off), *d_starts = (int *)(base + start_off), *d_count = (int *)(base + count_off);
    int *d_first = (int *)(base + first_off), *d_hit = (int *)(base + hit_off), *d_fit = (int *)(base + fit_off);
    unsigned long long *d_words = (unsigned long long *)(base + word_off);
    long long *d_lens = (long long *)(base + len_off), *d_offs = (long long *)(base + off_off);
    const unsigned trace_groups = (unsigned)std::min<long long>(kMaxTraceGroups, (bound + 3) / 4);
    hipStream_t st = ctx->stream;
    { VKX_TIMED(ctx, "k_contour_label_tiles"); k_contour_label_tiles<<<(unsigned)tiles, kBlock, 0, st>>>(d_recs, n_masks, d_labels); }
    { VKX_TIMED(ctx, "k_contour_merge"); k_contour_merge<<<(unsigned)tiles, kBlock, 0, st>>>(d_recs, n_masks, d_labels); }
    { VKX_TIMED(ctx, "k_contour_flags"); k_contour_flags<<<vkx_blocks((size_t)words, kBlock / 64), kBlock, 0, st>>>(d_recs, n_masks, (int)words, d_labels, d_words); }
    { VKX_TIMED(ctx, "k_contour_compact"); k_contour_compact<<<n_masks, kBlock, 0, st>>>(d_recs, d_words, d_starts, d_count); }
    { VKX_TIMED(ctx, "k_contour_mask_scan"); k_contour_mask_scan<<<1, kScanBlock, 0, st>>>(n_masks, d_count, d_first, d_hit); }
    { VKX_TIMED(ctx, "k_contour_trace_count"); k_contour_trace<false><<<trace_groups, kBlock, 0, st>>>(d_recs, n_masks, method, d_first, d_starts, d_lens, d_offs, d_hit, d_fit, (int2 *)points); }
    { VKX_TIMED(ctx, "k_contour_offsets"); k_contour_offsets<<<1, kScanBlock, 0, st>>>(n_masks, d_first, d_lens, d_offs, d_hit, cap_contours, cap_points, d_fit, n_contours, contour_len, contour_off, (long long *)totals, status); }
    { VKX_TIMED(ctx, "k_contour_trace_write"); k_contour_trace<true><<<trace_groups, kBlock, 0, st>>>(d_recs, n_masks, method, d_first, d_starts, d_lens, d_offs, d_hit, d_fit, (int2 *)points); }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
