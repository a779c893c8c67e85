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
//   k_region_mask_outline  one lane per (edge, major step) of every polygon of every region: the LINE_8 outline pixel, its
//                          polygon's bit (o 1, d 2, r 4) ORed into the region's bit plane.
//   k_region_mask_spans    one wave per (polygon, scanline): the even-odd spans, the same bit ORed lane-parallel.
//   k_region_mask_resolve  one lane a pixel of a region's box: the formula against T; every byte of the output is written once.
// The edge walk and the crossing ranking are vkx_poly_edges.h's, shared with vkx_fill_poly_mask_u8 / vkx_paint_polys_dev: the
// rasters are theirs pixel for pixel.  The bit planes pack four pixels a 32-bit word (bits are set with word atomics; the
// planes are context scratch, zeroed by one memset a call).  Small, latency-bound kernels; plain vector stores only.
#include "vkx_internal.h"
#include "vkx_poly_edges.h"

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

struct MaskItem {                                // one (polygon, scanline) pair
    int edge_begin, edge_end;
    int y;                                       // BB-relative
    int rec, bit;
};

__device__ __forceinline__ void set_bit(unsigned *__restrict__ bits, const MaskRec &r, int y, int x, int bit)
{
    const int idx = y * r.w + x;                 // h, w <= 32767: below 2^30
    atomicOr(&bits[r.bits_off + (idx >> 2)], (unsigned)bit << ((idx & 3) * 8));
}

// edges carry BB-relative coordinates, e.pad the region and e.poly the bit of their polygon
__global__ void __launch_bounds__(256) k_region_mask_outline(const PolyEdge *__restrict__ edges, int nedges, int total_steps,
                                                             const MaskRec *__restrict__ recs, unsigned *__restrict__ bits)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total_steps) return;
    const PolyEdge e = vkp::edge_of_step(edges, nedges, t);
    int x, y;
    vkp::edge_pixel(e, t, x, y);
    const MaskRec r = recs[e.pad];
    if ((unsigned)x < (unsigned)r.w && (unsigned)y < (unsigned)r.h) set_bit(bits, r, y, x, e.poly);
}

__global__ void __launch_bounds__(256) k_region_mask_spans(const PolyEdge *__restrict__ edges, const MaskItem *__restrict__ items,
                                                           int n_items, const MaskRec *__restrict__ recs,
                                                           unsigned *__restrict__ bits, int *__restrict__ overflow)
{
    __shared__ long long xs_all[4][kPaintCross];
    __shared__ long long sorted_all[4][kPaintCross];
    __shared__ int count_all[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int it = blockIdx.x * 4 + wave;
    const long long *sorted = sorted_all[wave];
    if (lane == 0) count_all[wave] = 0;
    __syncthreads();
    const bool live = it < n_items;
    MaskItem item = {0, 0, 0, 0, 0};
    if (live) item = items[it];
    int n = vkp::wave_crossings(edges, item.edge_begin, item.edge_end, item.y, xs_all[wave], &count_all[wave], lane);
    if (n > kPaintCross) {
        if (lane == 0) atomicExch(overflow, 1);
        n = 0;
    }
    vkp::wave_rank(xs_all[wave], sorted_all[wave], n, lane);
    if (!live) return;
    const MaskRec r = recs[item.rec];
    if ((unsigned)item.y >= (unsigned)r.h) return;
    for (int a = 0; a + 1 < n; a += 2) {
        long long x1, x2;
        vkp::span_of(sorted, a, r.w, x1, x2);
        for (long long x = x1 + lane; x <= x2; x += 64) set_bit(bits, r, item.y, (int)x, item.bit);
    }
}

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
    bool may_overflow = false;
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
            may_overflow = may_overflow || cnt[k] > kPaintCross;
        }
        recs[i] = MaskRec{words, g.dst_off, g.up, g.left, h, w};
        words += (area + 3) >> 2;
        groups = std::max(groups, std::min(kRegionGroups, ((w + 63) / 64) * ((h + 3) / 4)));
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++)
        VKX_REQUIRE(ranges[i].first >= ranges[i - 1].second, "destinations overlap one another");
    VKX_REQUIRE(total_pts < 0x3fffffff, "too many vertices");

    // the edge table of every polygon in BB-relative coordinates, and its (polygon, scanline) items
    std::vector<PolyEdge> edges((size_t)total_pts);
    std::vector<MaskItem> items;
    std::vector<int32_t> rel;
    long long steps = 0;
    size_t e_base = 0;
    for (int i = 0; i < n_regions; i++) {
        const vkx_region_masks_rec &g = regions_host[i];
        const int off[3] = {g.o_off, g.d_off, g.r_off}, cnt[3] = {g.o_cnt, g.d_cnt, g.r_cnt};
        for (int k = 0; k < 3; k++) {
            rel.resize((size_t)cnt[k] * 2);
            for (int j = 0; j < cnt[k]; j++) {
                rel[2 * (size_t)j] = pts_host[2 * ((size_t)off[k] + j)] - g.left;
                rel[2 * (size_t)j + 1] = pts_host[2 * ((size_t)off[k] + j) + 1] - g.up;
            }
            int ymin = INT_MAX, ymax = INT_MIN;
            build_edges(rel.data(), cnt[k], 1 << k, edges.data() + e_base, &steps, &ymin, &ymax);
            VKX_REQUIRE(steps < 0x7fffffff, "polygon outlines too long");
            for (size_t j = e_base; j < e_base + (size_t)cnt[k]; j++) edges[j].pad = i;
            for (int y = ymin; y < ymax; y++) items.push_back(MaskItem{(int)e_base, (int)e_base + cnt[k], y, i, 1 << k});
            e_base += (size_t)cnt[k];
        }
    }

    vkx_tables tab(ctx);             // behind the overflow flag's 256 bytes of ctx->rm_tables
    const size_t r_off = tab.add(sizeof(MaskRec) * recs.size()), e_off = tab.add(sizeof(PolyEdge) * edges.size());
    const size_t i_off = tab.add(sizeof(MaskItem) * items.size());
    int rc = vkx_scratch_reserve(ctx, &ctx->rm_tables, std::max(256 + vkx_align256(tab.bytes), (size_t)64 << 10));
    if (rc) return rc;
    const size_t bits_bytes = (size_t)words * 4;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->rm_bits, bits_bytes))) return rc;
    unsigned char *base = (unsigned char *)ctx->rm_tables.ptr;
    int *overflow = (int *)base;
    const MaskRec *d_recs = (const MaskRec *)(base + 256 + r_off);
    const PolyEdge *d_edges = (const PolyEdge *)(base + 256 + e_off);
    const MaskItem *d_items = (const MaskItem *)(base + 256 + i_off);
    unsigned *bits = (unsigned *)ctx->rm_bits.ptr;
    // The three tables travel through the context's page-locked ring as ONE asynchronous copy: the call returns with its kernels
    // queued.  A polygon of at most kPaintCross vertices cannot cross a scanline more often than the span kernel holds, so only
    // calls with larger polygons read the overflow flag back (and synchronise for it).
    vkx_device_guard guard(ctx);
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<MaskRec>(r_off), recs.data(), sizeof(MaskRec) * recs.size());
    memcpy(tab.at<PolyEdge>(e_off), edges.data(), sizeof(PolyEdge) * edges.size());
    if (!items.empty()) memcpy(tab.at<MaskItem>(i_off), items.data(), sizeof(MaskItem) * items.size());
    if ((rc = tab.copy_to(base + 256))) return rc;
    if (may_overflow) VKX_HIP(hipMemsetAsync(overflow, 0, sizeof(int), ctx->stream));      // (only such calls can set it, and only they read it)
    VKX_HIP(hipMemsetAsync(bits, 0, bits_bytes, ctx->stream));
    { VKX_TIMED(ctx, "k_region_mask_outline"); k_region_mask_outline<<<vkx_blocks((size_t)steps, 256), 256, 0, ctx->stream>>>(d_edges, (int)total_pts, (int)steps, d_recs, bits); }
    VKX_LAUNCH_CHECK();
    // (a page whose polygons are all flat has no scanline item: the launch stays, one idle workgroup, so that the launches of a
    //  call do not depend on its regions)
    { VKX_TIMED(ctx, "k_region_mask_spans"); k_region_mask_spans<<<vkx_blocks(items.size(), 4), 256, 0, ctx->stream>>>(d_edges, d_items, (int)items.size(), d_recs, bits, overflow); }
    VKX_LAUNCH_CHECK();
    { VKX_TIMED(ctx, "k_region_mask_resolve"); k_region_mask_resolve<<<dim3(n_regions, groups), 256, 0, ctx->stream>>>(d_recs, bits, text_mask, text_mask_step, dst); }
    VKX_LAUNCH_CHECK();
    if (!may_overflow) return VKX_OK;
    int flag = 0;
    VKX_HIP(hipMemcpyAsync(&flag, overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    VKX_HIP(hipStreamSynchronize(ctx->stream));
    if (flag) {
        vkx_set_error("a polygon has more than %d edge crossings on one scanline", kPaintCross);
        return VKX_ERR_UNSUPPORTED;
    }
    return VKX_OK;
}
