// The pixel half of PageTextRegionStep on gfx950 (reference: pipeline/text_detection/page_text_region.py:560-656
// TextRegionFlattener.build_flattened_text_regions, :109-166 the resize and the post-rotation of a FlattenedTextRegion,
// :732-856 build_background_image_for_stacking and stack_flattened_text_regions).
//
// Per text region the reference cuts the region out of the page under its mask, rotates image and mask, trims both to the
// rotated mask's external box, resizes both, may rotate again and blits the result into a striped page.  A page has tens to
// hundreds of regions of a few thousand pixels each: per-region launches are all dispatch.  Here every operation takes ALL
// regions of a page in ONE launch, its per-region records staged as one table (vkx_tables, one copy out of the ring):
//   k_region_warp     cv.warpAffine of N (image, mask) pairs; blockIdx.x is the pair, the workgroups of a pair (blockIdx.y)
//                     stride over its 64 x 4 tiles.  The coordinate is vkd::CoordAffine's, the pixel vkd::sample_taps_u8's:
//                     the arithmetic of vkx_warp_affine_u8_dev.  With `extract` an image tap is read as 0 where the source
//                     mask is 0 (Mask.extract_image, fused).  A pair writes a WINDOW of its warped plane: the trim.
//   k_region_extent   one workgroup a mask: first / last non-zero row and column, LDS min / max.
//   k_region_resize   cv.resize INTER_CUBIC of N pairs, the tables of every pair in the staged block; the pixel is
//                     vkd::taps_pixel_u8's, the arithmetic of vkx_resize_cubic_u8_dev.  The mask is read as (m > 0) * 255
//                     and written as (v > 0).
//   k_region_stack    one lane a page pixel: the workgroup first lists the regions whose boxes meet its 64 x 16 tile in
//                     LDS, a pixel then takes the LAST region of the list that covers it with a set mask (the order of the
//                     reference's fills), or the background stripe; both planes are written whole, once.
// These kernels are small and latency-bound; every value is written with plain vector stores.
#include "vkx_internal.h"
#include "vkx_resize_pixel.h"
#include "vkx_warp.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace {

constexpr int kMaxPairs = 4096;
constexpr int kMaxSide = 32767;                 // cv.remap's source limit, kept for every plane here
constexpr int kPairGroups = 64;                 // at most this many workgroups stride over the tiles of one pair
constexpr int kStackList = 256;                 // regions a stack tile lists in LDS before it falls back to scanning them all

struct WarpRec {
    const uint8_t *img, *msk;                   // (img_off / msk_off < 0: that plane is not written)
    long long img_step, msk_step;
    double m[6];                                // CoordAffine's inverse matrix
    int sh, sw, up, left, dh, dw;
    long long img_off, msk_off;
};

struct ResizeRec {
    const uint8_t *img, *msk;
    long long img_step, msk_step;
    int sh, sw, dh, dw;
    long long img_off, msk_off;
    long long tab_off;                          // the pair's 4-tap block (vkd::pack_taps), bytes from the start of the staged block
};

struct ExtentRec { long long off; int h, w; };

struct StackRec { const uint8_t *img, *msk; int h, w, up, left; };

template <bool kExtract>
__global__ void __launch_bounds__(256) k_region_warp(const WarpRec *__restrict__ recs, uint8_t *__restrict__ dst)
{
    const WarpRec r = recs[blockIdx.x];
    vkd::CoordAffine coord;
#pragma unroll
    for (int i = 0; i < 6; i++) coord.m[i] = r.m[i];
    const int tiles_x = (r.dw + 63) >> 6, tiles = tiles_x * ((r.dh + 3) >> 2);
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
        const int x = (t % tiles_x) * 64 + lx, y = (t / tiles_x) * 4 + ly;
        if (x >= r.dw || y >= r.dh) continue;
        int X, Y;
        coord(x + r.left, y + r.up, X, Y);
        const uint8_t *msk = r.msk;
        const long long ms = r.msk_step;
        if (r.msk_off >= 0) {
            uint8_t m;
            vkd::sample_taps_u8<1>([&](int sy, int sx, int) { return (int)msk[(ptrdiff_t)sy * ms + sx]; }, r.sh, r.sw, X, Y, &m);
            dst[r.msk_off + (ptrdiff_t)y * r.dw + x] = m;
        }
        if (r.img_off >= 0) {
            const uint8_t *img = r.img;
            const long long is = r.img_step;
            uint8_t px[3];
            vkd::sample_taps_u8<3>(
                [&](int sy, int sx, int k) {
                    if (kExtract && msk[(ptrdiff_t)sy * ms + sx] == 0) return 0;
                    return (int)img[(ptrdiff_t)sy * is + (ptrdiff_t)sx * 3 + k];
                },
                r.sh, r.sw, X, Y, px);
            uint8_t *o = dst + r.img_off + ((ptrdiff_t)y * r.dw + x) * 3;
            o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
        }
    }
}

// grid: one workgroup a mask; out[mask] = (up, down, left, right), or -1 four times for a mask without a set pixel
__global__ void __launch_bounds__(256) k_region_extent(const ExtentRec *__restrict__ recs, const uint8_t *__restrict__ masks,
                                                       int4 *__restrict__ out)
{
    __shared__ int lo_y, hi_y, lo_x, hi_x;
    const ExtentRec r = recs[blockIdx.x];
    if (threadIdx.x == 0) { lo_y = lo_x = INT_MAX; hi_y = hi_x = -1; }
    __syncthreads();
    const uint8_t *m = masks + r.off;
    int ay = INT_MAX, by = -1, ax = INT_MAX, bx = -1;
    const int n = r.h * r.w;                    // h, w <= 32767: below 2^30
    for (int i = threadIdx.x; i < n; i += 256) {
        if (m[i]) {
            const int y = i / r.w, x = i - y * r.w;
            ay = min(ay, y); by = max(by, y); ax = min(ax, x); bx = max(bx, x);
        }
    }
    if (by >= 0) { atomicMin(&lo_y, ay); atomicMax(&hi_y, by); atomicMin(&lo_x, ax); atomicMax(&hi_x, bx); }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = hi_y < 0 ? make_int4(-1, -1, -1, -1) : make_int4(lo_y, hi_y, lo_x, hi_x);
}

__global__ void __launch_bounds__(256) k_region_resize(const ResizeRec *__restrict__ recs, const unsigned char *__restrict__ tabs,
                                                       uint8_t *__restrict__ dst)
{
    const ResizeRec r = recs[blockIdx.x];
    const vkd::TapView<short> tab(tabs + r.tab_off, 4, r.dh, r.dw);
    const int tiles_x = (r.dw + 63) >> 6, tiles = tiles_x * ((r.dh + 3) >> 2);
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
        const int x = (t % tiles_x) * 64 + lx, y = (t / tiles_x) * 4 + ly;
        if (x >= r.dw || y >= r.dh) continue;
        const int x0 = tab.xofs[x], y0 = tab.yofs[y];
        const uint8_t *msk = r.msk;
        const long long ms = r.msk_step;
        if (r.msk_off >= 0) {
            uint8_t m;
            vkd::taps_pixel_u8<1, 4>([&](int sy, int b) { return msk[(ptrdiff_t)sy * ms + b] ? 255 : 0; }, r.sh, r.sw, x0, y0,
                                     tab.xcoef + 4 * x, tab.ycoef + 4 * y, &m);
            dst[r.msk_off + (ptrdiff_t)y * r.dw + x] = m ? 1 : 0;
        }
        if (r.img_off >= 0) {
            const uint8_t *img = r.img;
            const long long is = r.img_step;
            uint8_t px[3];
            vkd::taps_pixel_u8<3, 4>([&](int sy, int b) { return (int)img[(ptrdiff_t)sy * is + b]; }, r.sh, r.sw, x0, y0, tab.xcoef + 4 * x,
                                     tab.ycoef + 4 * y, px);
            uint8_t *o = dst + r.img_off + ((ptrdiff_t)y * r.dw + x) * 3;
            o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
        }
    }
}

// grid: (ceil(w / 64), ceil(h / 16)); a lane walks four rows of its column
__global__ void __launch_bounds__(256) k_region_stack(const StackRec *__restrict__ recs, int n, uint8_t *__restrict__ image,
                                                      uint8_t *__restrict__ mask, int h, int w)
{
    __shared__ int listed, list[kStackList];
    const int tx0 = blockIdx.x * 64, ty0 = blockIdx.y * 16;
    if (threadIdx.x == 0) listed = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const StackRec &r = recs[i];
        if (r.left < tx0 + 64 && r.left + r.w > tx0 && r.up < ty0 + 16 && r.up + r.h > ty0) {
            const int k = atomicAdd(&listed, 1);
            if (k < kStackList) list[k] = i;
        }
    }
    __syncthreads();
    const int m = listed;                       // (uniform)
    const bool all = m > kStackList;            // too many for the list: every region is a candidate
    const int cand = all ? n : m;
    const int x = tx0 + (threadIdx.x & 63);
    if (x >= w) return;
    for (int rr = 0; rr < 4; rr++) {
        const int y = ty0 + 4 * rr + (threadIdx.x >> 6);
        if (y >= h) continue;
        int best = -1;
        ptrdiff_t at = 0;
        for (int j = 0; j < cand; j++) {
            const int i = all ? j : list[j];
            if (i < best) continue;
            const StackRec &r = recs[i];
            const int ry = y - r.up, rx = x - r.left;
            if ((unsigned)ry < (unsigned)r.h && (unsigned)rx < (unsigned)r.w) {
                const ptrdiff_t p = (ptrdiff_t)ry * r.w + rx;
                if (r.msk[p]) { best = i; at = p; }
            }
        }
        const ptrdiff_t o = (ptrdiff_t)y * w + x;
        uint8_t *px = image + o * 3;
        if (best >= 0) {
            const uint8_t *s = recs[best].img + at * 3;
            px[0] = s[0]; px[1] = s[1]; px[2] = s[2];
        } else {
            const int c = (x + y) % 3;          // build_background_image_for_stacking: channel (y + x) % 3 is 255
            px[0] = c == 0 ? 255 : 0; px[1] = c == 1 ? 255 : 0; px[2] = c == 2 ? 255 : 0;
        }
        mask[o] = best >= 0 ? 1 : 0;
    }
}

// the source planes of a pair and where it writes, against the contract of vkx.h; need_mask: the mask is read even if unwritten
int check_pair(const uint8_t *src_image, const uint8_t *src_mask, long long image_step, long long mask_step, int sh, int sw,
               int dh, int dw, long long image_off, long long mask_off, bool need_mask, const uint8_t *dst, size_t dst_bytes,
               std::vector<std::pair<long long, long long>> *ranges)
{
    VKX_REQUIRE(image_off >= 0 || mask_off >= 0, "a pair that writes neither plane");
    VKX_REQUIRE(sh >= 1 && sw >= 1 && sh <= kMaxSide && sw <= kMaxSide, "source side outside 1 .. 32767");
    VKX_REQUIRE(dh >= 1 && dw >= 1 && dh <= kMaxSide && dw <= kMaxSide, "destination side outside 1 .. 32767");
    const long long mask_bytes = (long long)dh * dw;
    if (mask_off >= 0 || (need_mask && image_off >= 0)) {
        VKX_REQUIRE(src_mask != nullptr, "NULL source mask");
        VKX_REQUIRE_PITCH(mask_step, (ptrdiff_t)sw, sh);
        VKX_REQUIRE_DISJOINT(src_mask, sh, (ptrdiff_t)mask_step, (size_t)sw, dst, 1, 0, dst_bytes);
    }
    if (mask_off >= 0) {
        VKX_REQUIRE((unsigned long long)(mask_off + mask_bytes) <= dst_bytes, "destination mask outside dst");
        ranges->emplace_back(mask_off, mask_off + mask_bytes);
    }
    if (image_off >= 0) {
        VKX_REQUIRE(src_image != nullptr, "NULL source image");
        VKX_REQUIRE_PITCH(image_step, (ptrdiff_t)sw * 3, sh);
        VKX_REQUIRE((unsigned long long)(image_off + 3 * mask_bytes) <= dst_bytes, "destination image outside dst");
        VKX_REQUIRE_DISJOINT(src_image, sh, (ptrdiff_t)image_step, (size_t)sw * 3, dst, 1, 0, dst_bytes);
        ranges->emplace_back(image_off, image_off + 3 * mask_bytes);
    }
    return VKX_OK;
}

// gridDim.y of the pair kernels: the tile count of the LARGEST pair of the call, at most kPairGroups.  The grid is pairs x groups, so
// next to one large region every small one gets workgroups that find no tile and leave at once.  Deliberate: it keeps the
// launch free of a tile table that the host would have to build and stage per call, and an idle workgroup costs its dispatch only.
int pair_groups(int dh, int dw, int most) { return std::max(most, std::min(kPairGroups, ((dw + 63) / 64) * ((dh + 3) / 4))); }

}  // namespace

VKX_EXPORT int vkx_region_warp_dev(vkx_ctx *ctx, const vkx_region_warp_pair *pairs_host, int n_pairs, int extract, uint8_t *dst,
                                   size_t dst_bytes)
{
    VKX_REQUIRE(n_pairs >= 1 && n_pairs <= kMaxPairs, "1 .. 4096 pairs");
    VKX_REQUIRE(ctx && pairs_host && dst, "NULL argument");
    std::vector<std::pair<long long, long long>> ranges;
    int groups = 1;
    for (int i = 0; i < n_pairs; i++) {
        const vkx_region_warp_pair &p = pairs_host[i];
        if (int rc = check_pair(p.src_image, p.src_mask, p.src_image_step, p.src_mask_step, p.src_h, p.src_w, p.dst_h, p.dst_w,
                                p.dst_image_off, p.dst_mask_off, extract != 0, dst, dst_bytes, &ranges))
            return rc;
        VKX_REQUIRE(p.up >= 0 && p.left >= 0 && p.up <= kMaxSide - p.dst_h && p.left <= kMaxSide - p.dst_w,
                    "window outside a warped plane of at most 32767 px");
        groups = pair_groups(p.dst_h, p.dst_w, groups);
    }
    VKX_REQUIRE(!vkx_ranges_overlap(ranges), "destinations overlap one another");
    vkx_tables tab(ctx);
    int rc;
    if ((rc = tab.take(sizeof(WarpRec) * (size_t)n_pairs))) return rc;
    WarpRec *recs = tab.at<WarpRec>(0);
    for (int i = 0; i < n_pairs; i++) {
        const vkx_region_warp_pair &p = pairs_host[i];
        double forward[6];
        for (int k = 0; k < 6; k++) forward[k] = (double)p.m[k];
        const vkd::CoordAffine c = vkd::make_affine(forward);
        WarpRec &r = recs[i];
        r.img = p.src_image; r.msk = p.src_mask; r.img_step = p.src_image_step; r.msk_step = p.src_mask_step;
        for (int k = 0; k < 6; k++) r.m[k] = c.m[k];
        r.sh = p.src_h; r.sw = p.src_w; r.up = p.up; r.left = p.left; r.dh = p.dst_h; r.dw = p.dst_w;
        r.img_off = p.dst_image_off; r.msk_off = p.dst_mask_off;
    }
    if ((rc = tab.copy_to(&ctx->rf_tables, (size_t)64 << 10))) return rc;
    {
        VKX_TIMED(ctx, "k_region_warp");
        const dim3 grid(n_pairs, groups);
        if (extract) k_region_warp<true><<<grid, 256, 0, ctx->stream>>>((const WarpRec *)ctx->rf_tables.ptr, dst);
        else k_region_warp<false><<<grid, 256, 0, ctx->stream>>>((const WarpRec *)ctx->rf_tables.ptr, dst);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_region_extent_dev(vkx_ctx *ctx, const uint8_t *masks, size_t masks_bytes, const int64_t *offsets_host,
                                     const int32_t *shapes_host, int n_masks, int32_t *extents)
{
    VKX_REQUIRE(n_masks >= 1 && n_masks <= kMaxPairs, "1 .. 4096 masks");
    VKX_REQUIRE(ctx && masks && offsets_host && shapes_host && extents, "NULL argument");
    for (int i = 0; i < n_masks; i++) {
        const int h = shapes_host[2 * i], w = shapes_host[2 * i + 1];
        VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "mask side outside 1 .. 32767");
        VKX_REQUIRE(offsets_host[i] >= 0 && (unsigned long long)(offsets_host[i] + (long long)h * w) <= masks_bytes,
                    "mask outside the packed buffer");
    }
    VKX_REQUIRE(!vkx_planes_overlap(masks, 1, 0, masks_bytes, extents, 1, 0, sizeof(int32_t) * 4 * (size_t)n_masks),
                "the extents overlap the masks");
    vkx_tables tab(ctx);
    int rc;
    if ((rc = tab.take(sizeof(ExtentRec) * (size_t)n_masks))) return rc;
    ExtentRec *recs = tab.at<ExtentRec>(0);
    for (int i = 0; i < n_masks; i++) recs[i] = ExtentRec{offsets_host[i], shapes_host[2 * i], shapes_host[2 * i + 1]};
    if ((rc = tab.copy_to(&ctx->rf_tables, (size_t)64 << 10))) return rc;
    {
        VKX_TIMED(ctx, "k_region_extent");
        k_region_extent<<<n_masks, 256, 0, ctx->stream>>>((const ExtentRec *)ctx->rf_tables.ptr, masks, (int4 *)extents);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_region_resize_dev(vkx_ctx *ctx, const vkx_region_resize_pair *pairs_host, int n_pairs, uint8_t *dst,
                                     size_t dst_bytes)
{
    VKX_REQUIRE(n_pairs >= 1 && n_pairs <= kMaxPairs, "1 .. 4096 pairs");
    VKX_REQUIRE(ctx && pairs_host && dst, "NULL argument");
    std::vector<std::pair<long long, long long>> ranges;
    int groups = 1;
    size_t bytes = vkx_align256(sizeof(ResizeRec) * (size_t)n_pairs);
    std::vector<size_t> tab_off(n_pairs);
    for (int i = 0; i < n_pairs; i++) {
        const vkx_region_resize_pair &p = pairs_host[i];
        if (int rc = check_pair(p.src_image, p.src_mask, p.src_image_step, p.src_mask_step, p.src_h, p.src_w, p.dst_h, p.dst_w,
                                p.dst_image_off, p.dst_mask_off, false, dst, dst_bytes, &ranges))
            return rc;
        groups = pair_groups(p.dst_h, p.dst_w, groups);
        tab_off[i] = bytes;
        bytes += (vkd::pack_taps(4, false, p.src_h, p.src_w, p.dst_h, p.dst_w, nullptr) + 15) & ~(size_t)15;
    }
    VKX_REQUIRE(!vkx_ranges_overlap(ranges), "destinations overlap one another");
    vkx_tables tab(ctx);
    int rc;
    if ((rc = tab.take(bytes))) return rc;
    ResizeRec *recs = tab.at<ResizeRec>(0);
    for (int i = 0; i < n_pairs; i++) {
        const vkx_region_resize_pair &p = pairs_host[i];
        recs[i] = ResizeRec{p.src_image, p.src_mask, p.src_image_step, p.src_mask_step, p.src_h, p.src_w, p.dst_h, p.dst_w,
                            p.dst_image_off, p.dst_mask_off, (long long)tab_off[i]};
        vkd::pack_taps(4, false, p.src_h, p.src_w, p.dst_h, p.dst_w, tab.at<unsigned char>(tab_off[i]));
    }
    if ((rc = tab.copy_to(&ctx->rf_tables, (size_t)64 << 10))) return rc;
    {
        VKX_TIMED(ctx, "k_region_resize");
        k_region_resize<<<dim3(n_pairs, groups), 256, 0, ctx->stream>>>((const ResizeRec *)ctx->rf_tables.ptr,
                                                                          (const unsigned char *)ctx->rf_tables.ptr, dst);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_region_stack_dev(vkx_ctx *ctx, const vkx_region_stack_item *items_host, int n_items, uint8_t *page_image,
                                    uint8_t *page_mask, int h, int w)
{
    VKX_REQUIRE(n_items >= 0 && n_items <= kMaxPairs, "0 .. 4096 regions");
    VKX_REQUIRE(ctx && page_image && page_mask && (items_host || n_items == 0), "NULL argument");
    VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "page side outside 1 .. 32767");
    const size_t area = (size_t)h * w;
    VKX_REQUIRE(!vkx_planes_overlap(page_image, 1, 0, area * 3, page_mask, 1, 0, area), "the page planes overlap one another");
    for (int i = 0; i < n_items; i++) {
        const vkx_region_stack_item &p = items_host[i];
        VKX_REQUIRE(p.image && p.mask, "NULL region plane");
        VKX_REQUIRE(p.h >= 1 && p.w >= 1 && p.up >= 0 && p.left >= 0 && p.up <= h - p.h && p.left <= w - p.w,
                    "a region box outside the page");
        const size_t ra = (size_t)p.h * p.w;
        VKX_REQUIRE(!vkx_planes_overlap(p.image, 1, 0, ra * 3, page_image, 1, 0, area * 3) &&
                        !vkx_planes_overlap(p.image, 1, 0, ra * 3, page_mask, 1, 0, area) &&
                        !vkx_planes_overlap(p.mask, 1, 0, ra, page_image, 1, 0, area * 3) &&
                        !vkx_planes_overlap(p.mask, 1, 0, ra, page_mask, 1, 0, area),
                    "source and destination overlap (this operation cannot run in place)");
    }
    vkx_tables tab(ctx);
    int rc;
    if ((rc = tab.take(sizeof(StackRec) * (size_t)std::max(n_items, 1)))) return rc;
    StackRec *recs = tab.at<StackRec>(0);
    for (int i = 0; i < n_items; i++) {
        const vkx_region_stack_item &p = items_host[i];
        recs[i] = StackRec{p.image, p.mask, p.h, p.w, p.up, p.left};
    }
    if ((rc = tab.copy_to(&ctx->rf_tables, (size_t)64 << 10))) return rc;
    {
        VKX_TIMED(ctx, "k_region_stack");
        k_region_stack<<<dim3(vkx_blocks(w, 64), vkx_blocks(h, 16)), 256, 0, ctx->stream>>>((const StackRec *)ctx->rf_tables.ptr, n_items,
                                                                                             page_image, page_mask, h, w);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
