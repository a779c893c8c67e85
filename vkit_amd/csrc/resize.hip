// cv.resize(src, dsize, interpolation) on gfx950 (reference: Image.to_resized_image element/image.py:836-852,
// Mask.to_resized_mask element/mask.py:454-479, ScoreMap.to_resized_score_map element/score_map.py:616-640; first
// user on the path: the bottom layer of fill_page_inactive_region, pipeline/text_detection/page_distortion.py:146-161;
// every interpolation PageResizingStep samples, pipeline/text_detection/page_resizing.py:110-181 via utility/opt.py:125-148).
//
// The routing rule, the host-built axis tables and the blocks they travel in are vkx_resize_axes.h's, the arithmetic of a
// destination pixel vkx_resize_pixel.h's; here are the kernels -- the direct form, one lane a destination pixel on the 64 x 4
// tile of its workgroup, and the separable form of CUBIC / LANCZOS4 (k_resize_sep) --, the context's cache of table blocks and
// the dispatch.  The direct kernels are pure gathers, bound by HBM/L2 reads of the source (each source row is reused by
// ~4/scale destination rows).
#include "vkx_internal.h"
#include "vkx_resize_pixel.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>

namespace {

using vkd::clip_index;

// the destination pixel of a lane of the direct kernels (a 64 x 4 tile a workgroup); false: the lane is outside the plane
__device__ __forceinline__ bool lane_pixel(int dh, int dw, int &dy, int &dx)
{
    dx = blockIdx.x * 64 + (threadIdx.x & 63);
    dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    return dx < dw && dy < dh;
}

// INTER_LINEAR (KS = 2), INTER_CUBIC (4), INTER_LANCZOS4 (8) on uint8, tables as vkd::TapView lays them out
template <int CN, int KS>
__global__ void __launch_bounds__(256) k_resize_taps_u8(const uint8_t *__restrict__ src, int sh, int sw, ptrdiff_t sstride,
                                                        uint8_t *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                        const int *__restrict__ xofs, const short *__restrict__ xa,
                                                        const int *__restrict__ yofs, const short *__restrict__ yb)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    const auto load = [&](int y, int b) { return (int)(src + (ptrdiff_t)y * sstride)[b]; };      // (row pointer + int index)
    uint8_t *out = dst + (ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN;
    if constexpr (KS == 2) vkd::linear_pixel_u8<CN>(load, sh, sw, xofs[dx], yofs[dy], xa + dx * KS, yb + dy * KS, out);
    else vkd::taps_pixel_u8<CN, KS>(load, sh, sw, xofs[dx], yofs[dy], xa + dx * KS, yb + dy * KS, out);
}

template <int KS>
__global__ void __launch_bounds__(256) k_resize_taps_f32(const float *__restrict__ src, int sh, int sw, ptrdiff_t sstride,
                                                         float *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                         const int *__restrict__ xofs, const float *__restrict__ xc,
                                                         const int *__restrict__ yofs, const float *__restrict__ yc)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    dst[(ptrdiff_t)dy * dstride + dx] = vkd::taps_pixel_f32<KS>([&](int y, int x) { return src[(ptrdiff_t)y * sstride + x]; }, sh, sw,
                                                                xofs[dx], yofs[dy], xc + dx * KS, yc + dy * KS);
}

// the exact 2 x 2 shrink cv.resize routes to INTER_AREA
template <int CN>
__global__ void __launch_bounds__(256) k_resize_half_u8(const uint8_t *__restrict__ src, ptrdiff_t sstride,
                                                        uint8_t *__restrict__ dst, int dh, int dw, ptrdiff_t dstride)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    const uint8_t *p = src + (ptrdiff_t)(2 * dy) * sstride + (ptrdiff_t)(2 * dx) * CN;
    vkd::half_pixel_u8<CN>([&](int y, int x, int c) { return (int)p[y * sstride + x * CN + c]; }, dst + (ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN);
}

// INTER_NEAREST and INTER_NEAREST_EXACT (ifx .. ify0: the 16.16 step and start of x, then of y); CN = bytes per element
// (4 = one float32)
template <int CN>
__global__ void __launch_bounds__(256) k_resize_nearest_u8(const uint8_t *__restrict__ src, int sh, int sw, ptrdiff_t sstride,
                                                           uint8_t *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                           double ifx, double ify)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    const uint8_t *p = src + (ptrdiff_t)vkd::nearest_index(dy, ify, sh) * sstride + (ptrdiff_t)vkd::nearest_index(dx, ifx, sw) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) dst[(ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN + c] = p[c];
}

template <int CN>
__global__ void __launch_bounds__(256) k_resize_nearest_exact(const uint8_t *__restrict__ src, int sh, int sw, ptrdiff_t sstride,
                                                              uint8_t *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                              int ifx, int ifx0, int ify, int ify0)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    const uint8_t *p = src + (ptrdiff_t)vkd::nearest_exact_index(dy, ify, ify0, sh) * sstride +
                       (ptrdiff_t)vkd::nearest_exact_index(dx, ifx, ifx0, sw) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) dst[(ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN + c] = p[c];
}

// INTER_LINEAR_EXACT on uint8 (a LINEAR_EXACT block and its ranges), and INTER_LINEAR on float32
template <int CN>
__global__ void __launch_bounds__(256) k_resize_linear_exact_u8(const uint8_t *__restrict__ src, ptrdiff_t sstride,
                                                                uint8_t *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                                const int *__restrict__ xofs, const int *__restrict__ xw,
                                                                const int *__restrict__ yofs, const int *__restrict__ yw,
                                                                int xmin, int xmax, int ymin, int ymax)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    const int p[4] = {xmin, xmax, ymin, ymax};
    vkd::linear_exact_pixel_u8<CN>([&](int y, int below, int x, int c) { return (unsigned)(src + (ptrdiff_t)y * sstride + (below ? sstride : 0))[x * CN + c]; },
                                   vkd::LinearExactView{xofs, xw, yofs, yw}, p, dh, dw, dy, dx, dst + (ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN);
}

__global__ void __launch_bounds__(256) k_resize_linear_f32(const float *__restrict__ src, int sh, int sw, ptrdiff_t sstride,
                                                           float *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                           double scale_x, double scale_y)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    dst[(ptrdiff_t)dy * dstride + dx] = vkd::linear_pixel_f32([&](int y, int x) { return src[(ptrdiff_t)y * sstride + x]; }, sh, sw, dy, dx,
                                                              scale_x, scale_y);
}

// INTER_AREA: integer scale factors (box sums), and fractional ones (the weighted runs of an AREA block)
template <int CN, bool F32>
__global__ void __launch_bounds__(256) k_resize_area_fast(const void *__restrict__ src_, ptrdiff_t sstride, void *__restrict__ dst_,
                                                          int dh, int dw, ptrdiff_t dstride, int isx, int isy)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    if (F32) {
        const float *S = (const float *)src_ + (ptrdiff_t)(dy * isy) * sstride + (ptrdiff_t)(dx * isx);
        ((float *)dst_)[(ptrdiff_t)dy * dstride + dx] =
            vkd::area_fast_f32([&](int y, int x) { return S[(ptrdiff_t)y * sstride + x]; }, isx, isy);
    } else {
        const uint8_t *S = (const uint8_t *)src_ + (ptrdiff_t)(dy * isy) * sstride + (ptrdiff_t)(dx * isx) * CN;
        uint8_t *out = (uint8_t *)dst_ + (ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN;
#pragma unroll
        for (int c = 0; c < CN; c++)
            out[c] = vkd::area_fast_u8([&](int y, int x) { return (int)S[(ptrdiff_t)y * sstride + x * CN + c]; }, isx, isy);
    }
}

template <int CN, bool F32>
__global__ void __launch_bounds__(256) k_resize_area(const void *__restrict__ src_, ptrdiff_t sstride, void *__restrict__ dst_, int dh,
                                                     int dw, ptrdiff_t dstride, const vkd::AreaView t)
{
    int dy, dx;
    if (!lane_pixel(dh, dw, dy, dx)) return;
    if constexpr (F32) {
        vkd::area_pixel<1, true>([&](int y, int x, int) { return ((const float *)src_)[(ptrdiff_t)y * sstride + x]; }, t, dy, dx,
                                 (float *)dst_ + (ptrdiff_t)dy * dstride + dx);
    } else {
        vkd::area_pixel<CN, false>([&](int y, int x, int c) { return (float)((const uint8_t *)src_)[(ptrdiff_t)y * sstride + x * CN + c]; }, t,
                                   dy, dx, (uint8_t *)dst_ + (ptrdiff_t)dy * dstride + (ptrdiff_t)dx * CN);
    }
}

// zoom_in_blur (photometric/blur.py:264-316): uint16 accumulation of centred crops of enlarged copies, then
// uint8(clip((1 - alpha) * px + alpha * rint(acc / count))) in float64.
__global__ void __launch_bounds__(256) k_accumulate_crop(const uint8_t *__restrict__ src, ptrdiff_t sstride, int up, int left,
                                                         uint16_t *__restrict__ acc, int h, int wc, int cn, int init)
{
    const int xe = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (xe >= wc || y >= h) return;
    const uint16_t v = src[(ptrdiff_t)(up + y) * sstride + (ptrdiff_t)left * cn + xe];
    uint16_t *a = acc + (size_t)y * wc + xe;
    *a = init ? v : (uint16_t)(*a + v);      // numpy uint16 arithmetic wraps
}

__global__ void __launch_bounds__(256) k_zoom_finish(const uint8_t *__restrict__ src, ptrdiff_t sstride,
                                                     const uint16_t *__restrict__ acc, int h, int wc, int count, double w0,
                                                     double w1, uint8_t *__restrict__ dst, ptrdiff_t dstride)
{
    const int xe = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (xe >= wc || y >= h) return;
    const double t0 = w0 * (double)src[(ptrdiff_t)y * sstride + xe];
    const double mean = rint((double)acc[(size_t)y * wc + xe] / (double)count);   // np.round: half to even
    const double t1 = w1 * mean;
    double v = t0 + t1;
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    dst[(ptrdiff_t)y * dstride + xe] = (uint8_t)v;
}

// The table block of one resize geometry in device memory, from the ctx cache when the geometry was seen recently.  `pack` is
// a packer of vkx_resize_axes.h bound to the geometry -- pack(nullptr, meta) returns the block's bytes, pack(address, meta)
// writes it and the small host-side metadata that goes with it -- and runs on a miss only.  A block is one contiguous run of
// tables (its slot holds 256 bytes at least): a table starts where the one before it ends, so the coefficient tables of a tap
// block are aligned to 4 bytes only, which is all k_resize_sep and the direct kernels ask of them (int, short and float loads).
template <class Pack>
int cached_tables(vkx_ctx *ctx, const int (&key)[6], Pack pack, const unsigned char **block, const std::vector<int> **meta)
{
    vkx_ctx::ResizeTabs *slot = nullptr;
    for (auto &t : ctx->resize_tabs)
        if (std::equal(key, key + 6, t.key)) slot = &t;
    if (!slot) {
        slot = &ctx->resize_tabs[0];
        for (auto &t : ctx->resize_tabs)
            if (t.stamp < slot->stamp) slot = &t;
        slot->key[0] = -1;                        // invalid until the upload below has succeeded
        std::vector<int> m;
        // the block travels as ONE copy out of the page-locked ring (which keeps it alive): no copy per table, no stream
        // synchronisation per cache miss -- every page resizes to a geometry of its own
        vkx_tables tab(ctx);
        int rc = tab.take(pack(nullptr, &m));
        if (rc) return rc;
        pack(tab.at<unsigned char>(0), &m);
        if ((rc = tab.copy_to(&slot->buf, 256))) return rc;
        slot->meta.swap(m);
        std::copy(key, key + 6, slot->key);
    }
    slot->stamp = ++ctx->resize_clock;
    *block = (const unsigned char *)slot->buf.ptr;
    *meta = &slot->meta;
    return VKX_OK;
}

// ---- separable form of the CUBIC / LANCZOS4 gathers ------------------------------------------------------------------
// One workgroup = a 64 x 16 destination tile.  The source rows the tile's 16 destination rows reach (clipped to the
// image like the taps themselves) get their horizontal pass once, into LDS; the vertical pass reads them back.  The
// sums are the ones of the direct kernels above -- the horizontal sum of a source row does not depend on the
// destination row it is used for -- with K (rows / 16 + 1) multiply-adds per sample instead of K^2.  A tile that would
// need more than kSepRows source rows (a shrink by more than ~2x) is left to the direct kernels.
constexpr int kSepTileW = 64, kSepTileH = 16, kSepRows = 40;

template <typename T, typename CT, typename AT, int CN, int KS, int ROWS = kSepRows>
__global__ void __launch_bounds__(256) k_resize_sep(const T *__restrict__ src, int sh, int sw, ptrdiff_t sstride,
                                                    T *__restrict__ dst, int dh, int dw, ptrdiff_t dstride,
                                                    const int *__restrict__ xofs, const CT *__restrict__ xa,
                                                    const int *__restrict__ yofs, const CT *__restrict__ yb)
{
    __shared__ AT hbuf[ROWS * kSepTileW * CN];      // ROWS: 40, or 24 when no tile needs more (twice the workgroups per CU)
    constexpr int LEFT = KS / 2 - 1;          // taps s - LEFT .. s + KS / 2
    const int x0 = blockIdx.x * kSepTileW, y0 = blockIdx.y * kSepTileH;
    const int ylast = min(y0 + kSepTileH, dh) - 1;
    const int rmin = clip_index(yofs[y0] - LEFT, sh), rmax = clip_index(yofs[ylast] + KS / 2, sh);
    const int nrows = rmax - rmin + 1;
    // the vertical pass's row offsets and coefficients (wave-uniform) are fetched now: their latency hides under the horizontal pass
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int vt0[kSepTileH / 4];
    CT vb[kSepTileH / 4][KS];
#pragma unroll
    for (int i = 0; i < kSepTileH / 4; i++) {
        const int y = min(y0 + wave0 + 4 * i, dh - 1);
        vt0[i] = yofs[y] - LEFT;
#pragma unroll
        for (int k = 0; k < KS; k++) vb[i][k] = yb[y * KS + k];
    }
    if constexpr (sizeof(T) == 1) {
        // uint8: a thread keeps its column -- tap offset and the KS coefficients are loaded once, not once per source row --
        // and, when no tap is clipped, fetches the KS x CN consecutive source bytes of a row as whole dwords
        const int hx = threadIdx.x & 63, hdx = x0 + hx;
        if (hdx < dw) {
            const int s0 = xofs[hdx] - LEFT;
            int a[KS];
#pragma unroll
            for (int j = 0; j < KS; j++) a[j] = (int)xa[hdx * KS + j];
            const bool whole = s0 >= 0 && s0 + KS <= sw;
            constexpr int NB = KS * CN, ND = (NB + 3) / 4;
            typedef uint32_t u32_unaligned __attribute__((aligned(1)));
            // (the last dword may reach up to 3 bytes past the taps: only inside the row, never past the plane)
            const bool fast = whole && (ptrdiff_t)(s0 * CN + ND * 4) <= (ptrdiff_t)sw * CN;
            // The rows of a wavefront in batches of kBatch: all tap loads of a batch are issued before the first sum -- the tile used
            // to pay one memory round trip per source row (five in a row for a 1.05 x cubic: the kernel ran at the latency of its
            // loads, 13 % of the HBM roofline).
            constexpr int kBatch = 5;
            for (int rb = threadIdx.x >> 6; rb < nrows; rb += 4 * kBatch) {
                uint32_t w[kBatch][ND];
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const int r = min(rb + 4 * u, nrows - 1);
                    const uint8_t *row = (const uint8_t *)src + (ptrdiff_t)(rmin + r) * sstride;
#pragma unroll
                    for (int q = 0; q < ND; q++) w[u][q] = fast ? *(const u32_unaligned *)(row + (ptrdiff_t)s0 * CN + 4 * q) : 0u;
                }
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const int r = rb + 4 * u;
                    if (r >= nrows) break;
                    int hsum[CN];
#pragma unroll
                    for (int c = 0; c < CN; c++) hsum[c] = 0;
                    if (fast) {
#pragma unroll
                        for (int j = 0; j < KS; j++)
#pragma unroll
                            for (int c = 0; c < CN; c++) {
                                const int bb = j * CN + c;
                                hsum[c] += (int)((w[u][bb >> 2] >> (8 * (bb & 3))) & 0xffu) * a[j];
                            }
                    } else {
                        const uint8_t *row = (const uint8_t *)src + (ptrdiff_t)(rmin + r) * sstride;
#pragma unroll
                        for (int j = 0; j < KS; j++) {
                            const int sx = clip_index(s0 + j, sw) * CN;
#pragma unroll
                            for (int c = 0; c < CN; c++) hsum[c] += (int)row[sx + c] * a[j];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < CN; c++) hbuf[(r * kSepTileW + hx) * CN + c] = (AT)hsum[c];
                }
            }
        }
    } else {
    for (int idx = threadIdx.x; idx < nrows * kSepTileW; idx += 256) {
        const int r = idx / kSepTileW, lx = idx - r * kSepTileW, dx = x0 + lx;
        if (dx >= dw) continue;
        const T *row = src + (ptrdiff_t)(rmin + r) * sstride;
        const int s0 = xofs[dx] - LEFT;
        AT hsum[CN];
#pragma unroll
        for (int j = 0; j < KS; j++) {
            const int sx = clip_index(s0 + j, sw) * CN;
            const CT a = xa[dx * KS + j];
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const AT term = row[sx + c] * a;
                hsum[c] = j == 0 ? term : hsum[c] + term;
            }
        }
#pragma unroll
        for (int c = 0; c < CN; c++) hbuf[(r * kSepTileW + lx) * CN + c] = hsum[c];
    }
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, dx = x0 + lx;
    // the destination row is the same for the 64 lanes of a wavefront: row offsets and vertical coefficients are scalar
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if constexpr (sizeof(T) == 1 && CN == 3) {
        // RGB: four neighbouring lanes store their 12 bytes as three dwords (the group store of the fused chain kernel)
        typedef uint32_t u32_unaligned __attribute__((aligned(1)));
        const int tw = min(kSepTileW, dw - x0), full4 = (tw >> 2) << 2;
        const int right4 = min(lx + 1, 63) << 2;
#pragma unroll
        for (int i = 0; i < kSepTileH / 4; i++) {
            const int y = y0 + wave + 4 * i;
            if (y > ylast) break;
            const int t0 = vt0[i];
            int acc[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < KS; k++) {
                const AT *h = hbuf + ((clip_index(t0 + k, sh) - rmin) * kSepTileW + lx) * 3;
                const int b = (int)vb[i][k];
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] += __mul24((int)h[c], b);      // |h| < 2^20 (255 x the taps' |coefficients|): the 24-bit multiply is the 32-bit one, at full rate
            }
            uint32_t P = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int r = (acc[c] + (1 << 21)) >> 22;
                P |= (uint32_t)(r < 0 ? 0 : (r > 255 ? 255 : r)) << (8 * c);
            }
            const uint32_t Pn = (uint32_t)__builtin_amdgcn_ds_bpermute(right4, (int)P);
            if (dx >= dw) continue;
            uint8_t *orow = (uint8_t *)dst + (ptrdiff_t)y * dstride;
            const int m = lx & 3;
            if (lx < full4) {
                if (m < 3) *(u32_unaligned *)(orow + (ptrdiff_t)x0 * 3 + (lx >> 2) * 12 + m * 4) = (P >> (8 * m)) | (Pn << (24 - 8 * m));
            } else {
                uint8_t *o = orow + (ptrdiff_t)dx * 3;
                o[0] = (uint8_t)P; o[1] = (uint8_t)(P >> 8); o[2] = (uint8_t)(P >> 16);
            }
        }
        return;
    }
    if (dx >= dw) return;
#pragma unroll
    for (int i = 0; i < kSepTileH / 4; i++) {
        const int y = y0 + wave + 4 * i;
        if (y > ylast) break;
        const int t0 = vt0[i];
        AT acc[CN];
#pragma unroll
        for (int k = 0; k < KS; k++) {
            const AT *h = hbuf + ((clip_index(t0 + k, sh) - rmin) * kSepTileW + lx) * CN;
            const CT b = vb[i][k];
#pragma unroll
            for (int c = 0; c < CN; c++) {
                if constexpr (sizeof(T) == 1) {
                    const AT term = (AT)__mul24((int)h[c], (int)b);
                    acc[c] = k == 0 ? term : acc[c] + term;
                } else {
                    const AT term = h[c] * b;
                    acc[c] = k == 0 ? term : acc[c] + term;
                }
            }
        }
        T *out = dst + (ptrdiff_t)y * dstride + (ptrdiff_t)dx * CN;
#pragma unroll
        for (int c = 0; c < CN; c++) {
            if constexpr (sizeof(T) == 1) {
                const int r = ((int)(acc[c] + (1u << 21))) >> 22;
                out[c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
            } else {
                out[c] = acc[c];
            }
        }
    }
}

// can every 16-row destination tile keep its source rows in LDS?
// the most source rows a tile of the separable form needs; 0: more than kSepRows somewhere (the direct kernels take the call)
int separable_rows(const std::vector<int> &yofs, int sh, int dh, int ks)
{
    static const bool force_direct = vkx_env_on("VKX_RESIZE_DIRECT", 0);   // parity aid: the two forms must agree
    if (force_direct) return 0;
    const int left = ks / 2 - 1;
    auto clip = [sh](int v) { return v < 0 ? 0 : (v >= sh ? sh - 1 : v); };
    int most = 1;
    for (int y0 = 0; y0 < dh; y0 += kSepTileH) {
        const int ylast = std::min(y0 + kSepTileH, dh) - 1;
        most = std::max(most, clip(yofs[ylast] + ks / 2) - clip(yofs[y0] - left) + 1);
    }
    return most > kSepRows ? 0 : most;
}
constexpr int kSepRowsSmall = 24;

template <int KS>
void launch_sep_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t sstride, uint8_t *dst, int dh, int dw,
                   ptrdiff_t dstride, const int *xofs, const short *xa, const int *yofs, const short *yb, int rows = kSepRows)
{
    dim3 grid(vkx_blocks(dw, kSepTileW), vkx_blocks(dh, kSepTileH));
    if (rows <= kSepRowsSmall) {
        switch (cn) {
        case 1: k_resize_sep<uint8_t, short, unsigned, 1, KS, kSepRowsSmall><<<grid, 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, xofs, xa, yofs, yb); break;
        case 3: k_resize_sep<uint8_t, short, unsigned, 3, KS, kSepRowsSmall><<<grid, 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, xofs, xa, yofs, yb); break;
        default: k_resize_sep<uint8_t, short, unsigned, 4, KS, kSepRowsSmall><<<grid, 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, xofs, xa, yofs, yb); break;
        }
        return;
    }
    switch (cn) {
    case 1: k_resize_sep<uint8_t, short, unsigned, 1, KS><<<grid, 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, xofs, xa, yofs, yb); break;
    case 3: k_resize_sep<uint8_t, short, unsigned, 3, KS><<<grid, 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, xofs, xa, yofs, yb); break;
    default: k_resize_sep<uint8_t, short, unsigned, 4, KS><<<grid, 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, xofs, xa, yofs, yb); break;
    }
}

// f(std::integral_constant<int, CN>()) for the channel count of a call: the CN instance of a kernel template
template <class F>
void with_cn(int cn, F f)
{
    switch (cn) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
    }
}

dim3 direct_grid(int dh, int dw) { return dim3(vkx_blocks(dw, 64), vkx_blocks(dh, 4)); }

// CUBIC (KS = 4) and LANCZOS4 (8): the tap block from the cache, then the separable form where its tiles fit, else the direct one
template <int KS, class T>
int resize_taps(vkx_ctx *ctx, const T *src, int sh, int sw, int cn, ptrdiff_t sstride, T *dst, int dh, int dw, ptrdiff_t dstride)
{
    constexpr bool f32 = sizeof(T) == 4;
    using CT = typename std::conditional<f32, float, short>::type;
    const int key[6] = {KS, f32 ? 0 : 1, sh, sw, dh, dw};
    const unsigned char *block;
    const std::vector<int> *yofs_host;
    int rc = cached_tables(ctx, key, [&](unsigned char *out, std::vector<int> *yofs) { return vkd::pack_taps(KS, f32, sh, sw, dh, dw, out, yofs); },
                           &block, &yofs_host);
    if (rc) return rc;
    const vkd::TapView<CT> t(block, KS, dh, dw);
    VKX_TIMED(ctx, KS == 4 ? "k_resize_cubic" : "k_resize_lanczos4");
    const int rows = separable_rows(*yofs_host, sh, dh, KS);
    if constexpr (f32) {
        if (rows) k_resize_sep<float, float, float, 1, KS><<<dim3(vkx_blocks(dw, kSepTileW), vkx_blocks(dh, kSepTileH)), 256, 0, ctx->stream>>>(
                src, sh, sw, sstride, dst, dh, dw, dstride, t.xofs, t.xcoef, t.yofs, t.ycoef);
        else k_resize_taps_f32<KS><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, t.xofs, t.xcoef, t.yofs, t.ycoef);
    } else {
        if (rows) launch_sep_u8<KS>(ctx, src, sh, sw, cn, sstride, dst, dh, dw, dstride, t.xofs, t.xcoef, t.yofs, t.ycoef, rows);
        else with_cn(cn, [&](auto CN) {
            k_resize_taps_u8<CN, KS><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, sh, sw, sstride, dst, dh, dw, dstride, t.xofs, t.xcoef, t.yofs, t.ycoef);
        });
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

// interpolations shared by the uint8 and float32 entry points; elem = bytes per element for the nearest kernels
int resize_nearest(vkx_ctx *ctx, const vkd::ResizePlan &plan, const void *src, int sh, int sw, int elem, ptrdiff_t sstride_b, void *dst, int dh,
                   int dw, ptrdiff_t dstride_b)
{
    const bool exact = plan.mode == vkd::M_NEAREST_EXACT;
    VKX_TIMED(ctx, exact ? "k_resize_nearest_exact" : "k_resize_nearest");
    with_cn(elem, [&](auto CN) {
        if (exact) k_resize_nearest_exact<CN><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>((const uint8_t *)src, sh, sw, sstride_b, (uint8_t *)dst, dh, dw,
                                                                                         dstride_b, plan.p[0], plan.p[1], plan.p[2], plan.p[3]);
        else k_resize_nearest_u8<CN><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>((const uint8_t *)src, sh, sw, sstride_b, (uint8_t *)dst, dh, dw, dstride_b,
                                                                                plan.scale_x, plan.scale_y);
    });
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

template <bool F32>
int resize_area(vkx_ctx *ctx, const vkd::ResizePlan &plan, const void *src, int sh, int sw, int cn, ptrdiff_t sstride, void *dst, int dh, int dw,
                ptrdiff_t dstride)
{
    if (plan.mode == vkd::M_AREA_FAST) {
        VKX_TIMED(ctx, "k_resize_area_fast");
        with_cn(cn, [&](auto CN) {
            k_resize_area_fast<CN, F32><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, sstride, dst, dh, dw, dstride, plan.p[0], plan.p[1]);
        });
        VKX_LAUNCH_CHECK();
        return VKX_OK;
    }
    std::unique_ptr<vkd::AreaTabs> tabs;      // built on a cache miss only
    const int key[6] = {103, 0, sh, sw, dh, dw};
    const unsigned char *block;
    const std::vector<int> *n;                // the entry counts of x and y
    int rc = cached_tables(ctx, key, [&](unsigned char *out, std::vector<int> *counts) {
        if (!tabs) tabs.reset(new vkd::AreaTabs(sh, sw, dh, dw, plan.scale_x, plan.scale_y));
        *counts = {(int)tabs->x.si.size(), (int)tabs->y.si.size()};
        return tabs->pack(out);
    }, &block, &n);
    if (rc) return rc;
    VKX_TIMED(ctx, "k_resize_area");
    with_cn(cn, [&](auto CN) {
        k_resize_area<CN, F32><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, sstride, dst, dh, dw, dstride, vkd::AreaView(block, dh, dw, (*n)[0], (*n)[1]));
    });
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

// the refusals of the routing rule, in the words of the exported calls
int refuse(const vkd::ResizePlan &plan, int interpolation)
{
    if (plan.mode == vkd::M_REFUSED_AREA_ENLARGES) vkx_set_error("INTER_AREA is implemented for shrinking only (the reference samples it only then)");
    else vkx_set_error("unknown interpolation code %d", interpolation);
    return VKX_ERR_UNSUPPORTED;
}

} // namespace

VKX_EXPORT int vkx_resize_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride, uint8_t *dst,
                                 int dh, int dw, ptrdiff_t dst_stride, int interpolation)
{
    VKX_REQUIRE_PITCH(src_stride, (ptrdiff_t)sw * cn, sh);
    VKX_REQUIRE_PITCH(dst_stride, (ptrdiff_t)dw * cn, dh);
    VKX_REQUIRE_DISJOINT(src, sh, src_stride, (size_t)sw * cn, dst, dh, dst_stride, (size_t)dw * cn);
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "bad shape");
    VKX_REQUIRE(cn == 1 || cn == 3 || cn == 4, "1, 3 or 4 channels");
    vkd::ResizePlan plan = vkd::plan_resize(false, interpolation, sh, sw, dh, dw);
    switch (plan.mode) {
    case vkd::M_TAPS:
        return plan.ks == 4 ? resize_taps<4>(ctx, src, sh, sw, cn, src_stride, dst, dh, dw, dst_stride)
                            : resize_taps<8>(ctx, src, sh, sw, cn, src_stride, dst, dh, dw, dst_stride);
    case vkd::M_NEAREST:
    case vkd::M_NEAREST_EXACT: return resize_nearest(ctx, plan, src, sh, sw, cn, src_stride, dst, dh, dw, dst_stride);
    case vkd::M_AREA_FAST:
    case vkd::M_AREA: return resize_area<false>(ctx, plan, src, sh, sw, cn, src_stride, dst, dh, dw, dst_stride);
    case vkd::M_LINEAR_EXACT_U8: {
        const int key[6] = {105, 0, sh, sw, dh, dw};
        const unsigned char *block;
        const std::vector<int> *range;
        int rc = cached_tables(ctx, key, [&](unsigned char *out, std::vector<int> *r) {
            r->resize(4);
            return vkd::pack_linear_exact(sh, sw, dh, dw, out, r->data());
        }, &block, &range);
        if (rc) return rc;
        const int *p = range->data();
        const vkd::LinearExactView t = vkd::LinearExactView::of(block, dh, dw);
        VKX_TIMED(ctx, "k_resize_linear_exact");
        with_cn(cn, [&](auto CN) {
            k_resize_linear_exact_u8<CN><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, src_stride, dst, dh, dw, dst_stride, t.xofs, t.xw, t.yofs, t.yw, p[0], p[1], p[2], p[3]);
        });
        break;
    }
    case vkd::M_HALF_U8: {
        VKX_TIMED(ctx, "k_resize_half");
        with_cn(cn, [&](auto CN) { k_resize_half_u8<CN><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, src_stride, dst, dh, dw, dst_stride); });
        break;
    }
    case vkd::M_LINEAR_U8: {
        // not cached: one copy of the block out of the ring, no synchronisation
        vkx_tables tab(ctx);
        int rc = tab.take(vkd::pack_taps(2, false, sh, sw, dh, dw, nullptr));
        if (rc) return rc;
        vkd::pack_taps(2, false, sh, sw, dh, dw, tab.at<unsigned char>(0));
        if ((rc = tab.copy_to(&ctx->misc))) return rc;
        const vkd::TapView<short> t(ctx->misc.ptr, 2, dh, dw);
        VKX_TIMED(ctx, "k_resize_linear");
        with_cn(cn, [&](auto CN) {
            k_resize_taps_u8<CN, 2><<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, sh, sw, src_stride, dst, dh, dw, dst_stride, t.xofs, t.xcoef, t.yofs, t.ycoef);
        });
        break;
    }
    default: return refuse(plan, interpolation);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_resize_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el, float *dst, int dh,
                                  int dw, ptrdiff_t dst_stride_el, int interpolation)
{
    VKX_REQUIRE_PITCH(src_stride_el, sw, sh);
    VKX_REQUIRE_PITCH(dst_stride_el, dw, dh);
    VKX_REQUIRE_DISJOINT(src, sh, src_stride_el * 4, (size_t)sw * 4, dst, dh, dst_stride_el * 4, (size_t)dw * 4);
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "bad shape");
    const vkd::ResizePlan plan = vkd::plan_resize(true, interpolation, sh, sw, dh, dw);
    switch (plan.mode) {
    case vkd::M_TAPS:
        return plan.ks == 4 ? resize_taps<4>(ctx, src, sh, sw, 1, src_stride_el, dst, dh, dw, dst_stride_el)
                            : resize_taps<8>(ctx, src, sh, sw, 1, src_stride_el, dst, dh, dw, dst_stride_el);
    case vkd::M_NEAREST:
    case vkd::M_NEAREST_EXACT: return resize_nearest(ctx, plan, src, sh, sw, 4, src_stride_el * 4, dst, dh, dw, dst_stride_el * 4);
    case vkd::M_AREA_FAST:
    case vkd::M_AREA: return resize_area<true>(ctx, plan, src, sh, sw, 1, src_stride_el, dst, dh, dw, dst_stride_el);
    case vkd::M_LINEAR_F32: {
        VKX_TIMED(ctx, "k_resize_linear");
        k_resize_linear_f32<<<direct_grid(dh, dw), 256, 0, ctx->stream>>>(src, sh, sw, src_stride_el, dst, dh, dw, dst_stride_el, plan.scale_x, plan.scale_y);
        VKX_LAUNCH_CHECK();
        return VKX_OK;
    }
    default: return refuse(plan, interpolation);
    }
}

VKX_EXPORT int vkx_resize_cubic_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                                       uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride)
{
    return vkx_resize_u8_dev(ctx, src, sh, sw, cn, src_stride, dst, dh, dw, dst_stride, VKX_INTER_CUBIC);
}

VKX_EXPORT int vkx_resize_cubic_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                                        float *dst, int dh, int dw, ptrdiff_t dst_stride_el)
{
    return vkx_resize_f32_dev(ctx, src, sh, sw, src_stride_el, dst, dh, dw, dst_stride_el, VKX_INTER_CUBIC);
}

VKX_EXPORT int vkx_zoom_in_blur_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                       const int32_t *sizes_hw_host, int n_sizes, double alpha, uint8_t *dst,
                                       ptrdiff_t dst_stride)
{
    VKX_REQUIRE_PITCH(src_stride, (ptrdiff_t)w * cn, h);
    VKX_REQUIRE_PITCH(dst_stride, (ptrdiff_t)w * cn, h);
    VKX_REQUIRE_DISJOINT(src, h, src_stride, (ptrdiff_t)w * cn, dst, h, dst_stride, (ptrdiff_t)w * cn);
    VKX_REQUIRE(ctx && src && dst && (n_sizes == 0 || sizes_hw_host), "NULL argument");
    VKX_REQUIRE(h > 0 && w > 0 && n_sizes >= 0, "bad shape");
    VKX_REQUIRE(cn == 1 || cn == 3 || cn == 4, "1, 3 or 4 channels");
    VKX_REQUIRE(n_sizes < 256, "too many zoom steps for a uint16 accumulator");
    size_t max_plane = 0;
    for (int i = 0; i < n_sizes; i++) {
        const int rh = sizes_hw_host[2 * i], rw = sizes_hw_host[2 * i + 1];
        VKX_REQUIRE(rh >= h && rw >= w, "zoom steps must not shrink the image");
        max_plane = std::max(max_plane, (size_t)rh * rw * cn);
    }
    const int wc = w * cn;
    int rc = vkx_scratch_reserve(ctx, &ctx->chain[0], max_plane + 256);
    if (rc) return rc;
    rc = vkx_scratch_reserve(ctx, &ctx->chain[1], (size_t)h * wc * sizeof(uint16_t));
    if (rc) return rc;
    uint8_t *big = (uint8_t *)ctx->chain[0].ptr;
    uint16_t *acc = (uint16_t *)ctx->chain[1].ptr;
    dim3 grid(vkx_blocks(wc, 64), vkx_blocks(h, 4));
    { VKX_TIMED(ctx, "k_accumulate_crop"); k_accumulate_crop<<<grid, 256, 0, ctx->stream>>>(src, src_stride, 0, 0, acc, h, wc, cn, 1); }
    VKX_LAUNCH_CHECK();
    for (int i = 0; i < n_sizes; i++) {
        const int rh = sizes_hw_host[2 * i], rw = sizes_hw_host[2 * i + 1];
        rc = vkx_resize_cubic_u8_dev(ctx, src, h, w, cn, src_stride, big, rh, rw, (ptrdiff_t)rw * cn);
        if (rc) return rc;
        { VKX_TIMED(ctx, "k_accumulate_crop"); k_accumulate_crop<<<grid, 256, 0, ctx->stream>>>(big, (ptrdiff_t)rw * cn, (rh - h) / 2, (rw - w) / 2, acc, h, wc, cn, 0); }
        VKX_LAUNCH_CHECK();
    }
    { VKX_TIMED(ctx, "k_zoom_finish"); k_zoom_finish<<<grid, 256, 0, ctx->stream>>>(src, src_stride, acc, h, wc, n_sizes + 1, 1 - alpha, alpha, dst, dst_stride); }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

