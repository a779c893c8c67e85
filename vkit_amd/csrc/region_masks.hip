// The bounding extended text-region masks of a page on gfx950 (reference: pipeline/text_detection/page_text_region.py:477-558
// TextRegionFlattener.get_bounding_extended_text_region_masks): the masks that build_flattened_text_regions (region_flatten.hip)
// starts from.
//
// Per text region the reference rasterises three polygons over the region's box BB -- the original polygon O, the (possibly
// dilated) polygon D and the bounding rectangular polygon R -- and combines them with the page's text mask T (the union of all
// original polygons) by two inversions, two count planes and an extraction.  Pixel by pixel that sequence is
//     out = (d and not (r and T and not o)) or (r and not T)
// (`other` is T copied under r and cleared under o; `trimmed` = d and not other; `non_text` = r and not T; out = trimmed or non_text).
// A page has tens to hundreds of regions of a few thousand pixels each, so all regions go through THREE launches:
//   k_region_mask_outline  vkp::k_outline over every polygon of every region, in BB-relative coordinates: the LINE_8 outline
//                          pixel, its polygon's bit (o 1, d 2, r 4) ORed into the region's bit plane.
//   k_region_mask_spans    vkp::k_spans: one wave per (polygon, scanline), the even-odd spans, the same bit ORed lane-parallel.
//   k_region_mask_resolve  one lane a pixel of a region's box: the formula against T; every byte of the output is written once.
// The raster is vkx_poly_raster.h's, shared with vkx_fill_poly_mask_u8 / vkx_paint_polys_dev (pixel for pixel theirs); what is
// here is its sink, BitSink.  The bit planes pack four pixels a 32-bit word (bits are set with word atomics; the planes are
// context scratch, zeroed by one memset a call).  Small, latency-bound kernels; plain vector stores only.
#include "vkx_internal.h"
#include "vkx_poly_raster.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace {

constexpr int kMaxRegions = 4096;
constexpr int kMaxSide = 32767;
constexpr int kRegionGroups = 64;                // at most this many workgroups stride over the tiles of one region

struct MaskRec {
    long long bits_off;                          // the region's bit plane, in words of the scratch block
    long long dst_off;
    int up, left, h, w;                          // BB
};

// The target of a polygon is its region (clipped to the region's box), its tag the bit of its plane.
struct BitSink {
    const MaskRec *recs;
    unsigned *bits;
    struct Row {
        unsigned *bits;
        MaskRec r;
        int w, y, bit;
        __device__ void operator()(int x) const { set(bits, r, y, x, bit); }
    };
    static __device__ __forceinline__ void set(unsigned *__restrict__ bits, const MaskRec &r, int y, int x, int bit)
    {
        const int idx = y * r.w + x;             // h, w <= 32767: below 2^30
        atomicOr(&bits[r.bits_off + (idx >> 2)], (unsigned)bit << ((idx & 3) * 8));
    }
    __device__ void pixel(const vkp::PolyEdge &e, int x, int y) const
    {
        const MaskRec r = recs[e.pad];
        if ((unsigned)x < (unsigned)r.w && (unsigned)y < (unsigned)r.h) set(bits, r, y, x, e.poly);
    }
    __device__ Row row(const vkp::Item &item) const
    {
        const MaskRec r = recs[item.target];
        return Row{bits, r, (unsigned)item.y < (unsigned)r.h ? r.w : 0, item.y, item.tag};
    }
};

// grid: (region, workgroups striding over the region's 64 x 4 tiles)
__global__ void __launch_bounds__(256) k_region_mask_resolve(const MaskRec *__restrict__ recs, const unsigned *__restrict__ bits,
                                                             const uint8_t *__restrict__ text_mask, ptrdiff_t text_step,
                                                             uint8_t *__restrict__ dst)
{
    const MaskRec r = recs[blockIdx.x];
    const int tiles_x = (r.w + 63) >> 6, tiles = tiles_x * ((r.h + 3) >> 2);
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
        const int x = (t % tiles_x) * 64 + lx, y = (t / tiles_x) * 4 + ly;
        if (x >= r.w || y >= r.h) continue;
        const int idx = y * r.w + x;
        const unsigned b = bits[r.bits_off + (idx >> 2)] >> ((idx & 3) * 8);
        const bool o = b & 1, d = b & 2, rr = b & 4;
        const bool T = text_mask[(ptrdiff_t)(r.up + y) * text_step + r.left + x] != 0;
        dst[r.dst_off + idx] = ((d && !(rr && T && !o)) || (rr && !T)) ? 1 : 0;
    }
}

}  // namespace

VKX_EXPORT int vkx_region_extend_masks_dev(vkx_ctx *ctx, const vkx_region_masks_rec *regions_host, int n_regions,
                                           const int32_t *pts_host, const uint8_t *text_mask, ptrdiff_t text_mask_step, int page_h,
                                           int page_w, uint8_t *dst, size_t dst_bytes)
{
    VKX_REQUIRE(n_regions >= 1 && n_regions <= kMaxRegions, "1 .. 4096 regions");
    VKX_REQUIRE(ctx && regions_host && pts_host && text_mask && dst, "NULL argument");
    VKX_REQUIRE(page_h >= 1 && page_w >= 1, "bad page shape");
    VKX_REQUIRE_PITCH(text_mask_step, page_w, page_h);
    VKX_REQUIRE(!vkx_planes_overlap(text_mask, page_h, text_mask_step, (size_t)page_w, dst, 1, 0, dst_bytes),
                "the text mask overlaps dst");
    std::vector<std::pair<long long, long long>> ranges;
    std::vector<MaskRec> recs((size_t)n_regions);
    long long total_pts = 0, words = 0;
    int groups = 1;
    for (int i = 0; i < n_regions; i++) {
        const vkx_region_masks_rec &g = regions_host[i];
        VKX_REQUIRE(g.up >= 0 && g.left >= 0 && g.up <= g.down && g.left <= g.right && g.down < page_h && g.right < page_w,
                    "a region box outside the page");
        const int h = g.down - g.up + 1, w = g.right - g.left + 1;
        VKX_REQUIRE(h <= kMaxSide && w <= kMaxSide, "a region box side outside 1 .. 32767");
        const long long area = (long long)h * w;
        VKX_REQUIRE(g.dst_off >= 0 && (unsigned long long)(g.dst_off + area) <= dst_bytes, "destination outside dst");
        ranges.emplace_back(g.dst_off, g.dst_off + area);
        const int off[3] = {g.o_off, g.d_off, g.r_off}, cnt[3] = {g.o_cnt, g.d_cnt, g.r_cnt};
        for (int k = 0; k < 3; k++) {
            VKX_REQUIRE(cnt[k] >= 1 && off[k] >= 0 && off[k] <= INT_MAX - cnt[k], "a polygon of fewer than 1 point, or a bad point range");
            for (int j = off[k]; j < off[k] + cnt[k]; j++) {
                const int x = pts_host[2 * (size_t)j], y = pts_host[2 * (size_t)j + 1];
                VKX_REQUIRE(x >= g.left && x <= g.right && y >= g.up && y <= g.down, "a polygon vertex outside its region box");
            }
            total_pts += cnt[k];
        }
        recs[i] = MaskRec{words, g.dst_off, g.up, g.left, h, w};
        words += (area + 3) >> 2;
        groups = std::max(groups, std::min(kRegionGroups, ((w + 63) / 64) * ((h + 3) / 4)));
    }
    VKX_REQUIRE(!vkx_ranges_overlap(ranges), "destinations overlap one another");
    // every polygon in BB-relative coordinates
    vkp::Raster<vkp::kPaintCross> raster;
    VKX_REQUIRE(raster.reserve(total_pts), "too many vertices");
    for (int i = 0; i < n_regions; i++) {
        const vkx_region_masks_rec &g = regions_host[i];
        const int off[3] = {g.o_off, g.d_off, g.r_off}, cnt[3] = {g.o_cnt, g.d_cnt, g.r_cnt};
        for (int k = 0; k < 3; k++)
            VKX_REQUIRE(raster.add(pts_host + 2 * (size_t)off[k], cnt[k], 1 << k, i, INT_MIN, INT_MAX, -g.left, -g.up), "polygon outlines too long");
    }

    vkx_tables tab(ctx);             // behind the overflow flag's 256 bytes of ctx->rm_tables
    const size_t r_off = tab.add(sizeof(MaskRec) * recs.size());
    raster.layout(tab);
    int rc = vkx_scratch_reserve(ctx, &ctx->rm_tables, std::max(256 + vkx_align256(tab.bytes), (size_t)64 << 10));
    if (rc) return rc;
    const size_t bits_bytes = (size_t)words * 4;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->rm_bits, bits_bytes))) return rc;
    unsigned char *base = (unsigned char *)ctx->rm_tables.ptr;
    int *overflow = (int *)base;
    const MaskRec *d_recs = (const MaskRec *)(base + 256 + r_off);
    unsigned *bits = (unsigned *)ctx->rm_bits.ptr;
    // The three tables travel through the context's page-locked ring as ONE asynchronous copy: the call returns with its kernels
    // queued unless a polygon could overflow (vkp::Raster).
    vkx_device_guard guard(ctx);
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<MaskRec>(r_off), recs.data(), sizeof(MaskRec) * recs.size());
    raster.stage(tab);
    if ((rc = tab.copy_to(base + 256))) return rc;
    VKX_HIP(hipMemsetAsync(bits, 0, bits_bytes, ctx->stream));
    // (a page whose polygons are all flat has no scanline item: the span launch stays, one idle workgroup, so that the launches
    //  of a call do not depend on its regions)
    if ((rc = raster.launch(ctx, base + 256, overflow, BitSink{d_recs, bits}, "k_region_mask_outline", "k_region_mask_spans", true))) return rc;
    { VKX_TIMED(ctx, "k_region_mask_resolve"); k_region_mask_resolve<<<dim3(n_regions, groups), 256, 0, ctx->stream>>>(d_recs, bits, text_mask, text_mask_step, dst); }
    VKX_LAUNCH_CHECK();
    return raster.finish(ctx, overflow, "a polygon");
}
