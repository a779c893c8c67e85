// Char binding on gfx950: the mask-overlap counts behind the reference's calculate_boxed_masks_intersected_ratio
// (pipeline/text_detection/page_text_region.py:189-227) for every (candidate, anchor) pair that
// PageTextRegionStep.strtree_query_intersected_polygons (:899-925) visits -- the pairing of precise polygons with disconnected
// text regions (:1115-1149) and the binding of a page's char polygons to its precise text regions (:1160-1216).
//
// A page has a few thousand chars of about 30 x 30 pixels and tens to hundreds of regions.  Every polygon is rasterised ONCE
// into a bit plane of its own (one bit a pixel, bit x & 31 of word x >> 5, rows padded to whole 32-bit words; the planes are
// context scratch, zeroed by one memset a call), and every pair ANDs two planes over the intersection of their boxes:
//   k_overlap_outline  vkp::k_outline over every polygon, in box-relative coordinates: the LINE_8 outline pixel ORed into the
//                      polygon's plane.
//   k_overlap_spans    vkp::k_spans: one wave per (polygon, scanline), the even-odd spans ORed lane-parallel.
//   k_overlap_count    one work item a polygon (its raster area) and one a pair (its intersected area): a lane takes a
//                      (row, word) of the candidate inside the window, funnel-shifts the two anchor words that cover it into place
//                      (v_alignbit_b32), masks the window's first and last word, ANDs and counts bits.  Items of at most 64
//                      (row, word) elements -- a char is about 30 rows of one word -- share a wave four at a time, 16 lanes each;
//                      a larger item takes a workgroup that strides over it.  The lanes' sums meet through __shfl_down (and LDS
//                      across the four waves of a workgroup); one lane writes the count with a plain vector store.  No atomics on
//                      the outputs: a rerun gives identical bytes.
// The raster is vkx_poly_raster.h's, pixel for pixel that of vkx_fill_poly_mask_u8; what is here is its sink, BitRowSink (the
// sibling of region_masks.hip's BitSink).  The second entry point, vkx_mask_overlap_counts_dev, serves masks that are not
// polygons: uint8 planes with row steps, one launch, the same reduction.
#include "vkx_internal.h"
#include "vkx_poly_raster.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int kMaxSide = 32767;
constexpr int kSmallElems = 64;                  // a work item of at most this many (row, word) elements takes 16 lanes
constexpr int kMaxMaskRecs = 65536;

struct PlaneRec {
    long long off;                               // the polygon's bit plane, in words of the scratch block
    int up, left, h, w;                          // its box
};
__host__ __device__ inline int row_words(int w) { return (w + 31) >> 5; }

struct WorkRec {
    int cand, anchor;                            // anchor < 0: the raster area of polygon `cand`
    int out;                                     // the index in counts
    int pad;
};

// The target of a polygon is its own plane (clipped to its box).
struct BitRowSink {
    const PlaneRec *planes;
    unsigned *bits;
    struct Row {
        unsigned *row;
        int w;
        __device__ void operator()(int x) const { atomicOr(&row[x >> 5], 1u << (x & 31)); }
    };
    __device__ void pixel(const vkp::PolyEdge &e, int x, int y) const
    {
        const PlaneRec p = planes[e.pad];
        if ((unsigned)x < (unsigned)p.w && (unsigned)y < (unsigned)p.h)
            atomicOr(&bits[p.off + (long long)y * row_words(p.w) + (x >> 5)], 1u << (x & 31));
    }
    __device__ Row row(const vkp::Item &item) const
    {
        const PlaneRec p = planes[item.target];
        const bool inside = (unsigned)item.y < (unsigned)p.h;
        return Row{bits + p.off + (inside ? (long long)item.y * row_words(p.w) : 0), inside ? p.w : 0};
    }
};

// The part of one work item that lane `lane` of `kLanes` takes.
template <int kLanes>
__device__ __forceinline__ unsigned item_bits(const PlaneRec *__restrict__ planes, const unsigned *__restrict__ bits, const WorkRec &wk,
                                              int lane)
{
    const PlaneRec c = planes[wk.cand];
    const int cw = row_words(c.w);
    unsigned acc = 0;
    if (wk.anchor < 0) {
        const unsigned *plane = bits + c.off;
        for (int e = lane; e < c.h * cw; e += kLanes) acc += __popc(plane[e]);      // h, w <= 32767: below 2^25 words
        return acc;
    }
    const PlaneRec a = planes[wk.anchor];
    // the window, in page coordinates (down and right exclusive)
    const int up = max(c.up, a.up), down = min(c.up + c.h, a.up + a.h);
    const int left = max(c.left, a.left), right = min(c.left + c.w, a.left + a.w);
    if (up >= down || left >= right) return 0;
    const int y0 = up - c.up, rows = down - up;                 // ... in the candidate's rows
    const int x0 = left - c.left, x1 = right - 1 - c.left;      // ... in the candidate's columns, inclusive
    const int j0 = x0 >> 5, nw = (x1 >> 5) - j0 + 1;
    const int dy = c.up - a.up, dx = c.left - a.left;           // anchor coordinate = candidate coordinate + (dx, dy)
    const int aw = row_words(a.w);
    for (int e = lane; e < rows * nw; e += kLanes) {
        const int r = e / nw, j = j0 + (e - r * nw);
        const int y = y0 + r;
        const unsigned cbits = bits[c.off + (long long)y * cw + j];
        // the candidate word's 32 pixels begin at anchor column ax: anchor words k and k + 1 cover them (either may lie outside
        // the anchor's row: no pixels there)
        const int ax = 32 * j + dx, k = ax >> 5;
        const unsigned *arow = bits + a.off + (long long)(y + dy) * aw;
        const unsigned lo = (unsigned)k < (unsigned)aw ? arow[k] : 0u;
        const unsigned hi = (unsigned)(k + 1) < (unsigned)aw ? arow[k + 1] : 0u;
        const unsigned abits = __builtin_amdgcn_alignbit(hi, lo, (unsigned)ax & 31u);
        const int first = max(x0 - 32 * j, 0), last = min(x1 - 32 * j, 31);
        const unsigned window = (0xffffffffu >> (31 - last)) & (0xffffffffu << first);
        acc += __popc(cbits & abits & window);
    }
    return acc;
}

// grid: the first n_large workgroups take one large item each (work[blockIdx.x]); every later workgroup takes 16 small items
// (work[n_large + 16 * b + group], 16 lanes each).
__global__ void __launch_bounds__(256) k_overlap_count(const PlaneRec *__restrict__ planes, const unsigned *__restrict__ bits,
                                                       const WorkRec *__restrict__ work, int n_work, int n_large,
                                                       int *__restrict__ counts)
{
    __shared__ unsigned part[4];
    if ((int)blockIdx.x < n_large) {
        const WorkRec wk = work[blockIdx.x];
        unsigned acc = item_bits<256>(planes, bits, wk, threadIdx.x);
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) counts[wk.out] = (int)(part[0] + part[1] + part[2] + part[3]);
        return;
    }
    const int it = n_large + ((int)blockIdx.x - n_large) * 16 + (threadIdx.x >> 4);
    const bool live = it < n_work;
    WorkRec wk = {0, -1, 0, 0};
    if (live) wk = work[it];
    unsigned acc = live ? item_bits<16>(planes, bits, wk, threadIdx.x & 15) : 0u;
    for (int d = 8; d > 0; d >>= 1) acc += __shfl_down(acc, d, 16);
    if (live && (threadIdx.x & 15) == 0) counts[wk.out] = (int)acc;
}

// ---- masks that are not polygons ---------------------------------------------------------------------------------------------
// grid: one workgroup a record, striding over the anchor's plane, the candidate's plane and the window
__global__ void __launch_bounds__(256) k_mask_overlap_count(const vkx_mask_overlap_rec *__restrict__ recs, long long *__restrict__ counts)
{
    __shared__ unsigned long long part[3][4];
    const vkx_mask_overlap_rec r = recs[blockIdx.x];
    unsigned long long acc[3] = {0, 0, 0};
    const int up = max(r.anchor_up, r.candidate_up), down = min(r.anchor_up + r.anchor_h, r.candidate_up + r.candidate_h);
    const int left = max(r.anchor_left, r.candidate_left), right = min(r.anchor_left + r.anchor_w, r.candidate_left + r.candidate_w);
    if (up < down && left < right) {
        const int ww = right - left, n = (down - up) * ww;      // sides <= 32767: below 2^30
        const uint8_t *a = r.anchor + (ptrdiff_t)(up - r.anchor_up) * r.anchor_step + (left - r.anchor_left);
        const uint8_t *c = r.candidate + (ptrdiff_t)(up - r.candidate_up) * r.candidate_step + (left - r.candidate_left);
        for (int e = threadIdx.x; e < n; e += 256) {
            const int y = e / ww, x = e - y * ww;
            acc[0] += (unsigned)(a[(ptrdiff_t)y * r.anchor_step + x] & c[(ptrdiff_t)y * r.candidate_step + x]);
        }
    }
    for (int e = threadIdx.x; e < r.anchor_h * r.anchor_w; e += 256) {
        const int y = e / r.anchor_w, x = e - y * r.anchor_w;
        acc[1] += r.anchor[(ptrdiff_t)y * r.anchor_step + x] != 0;
    }
    for (int e = threadIdx.x; e < r.candidate_h * r.candidate_w; e += 256) {
        const int y = e / r.candidate_w, x = e - y * r.candidate_w;
        acc[2] += r.candidate[(ptrdiff_t)y * r.candidate_step + x] != 0;
    }
    for (int k = 0; k < 3; k++) {
        for (int d = 32; d > 0; d >>= 1) acc[k] += __shfl_down(acc[k], d, 64);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        counts[3 * (long long)blockIdx.x + k] = (long long)(part[k][0] + part[k][1] + part[k][2] + part[k][3]);
    }
}

}  // namespace

VKX_EXPORT int vkx_poly_overlap_counts_dev(vkx_ctx *ctx, const vkx_poly_overlap_rec *polys_host, int n_polys, const int32_t *pts_host,
                                           const int32_t *pairs_host, int n_pairs, int32_t *counts)
{
    VKX_REQUIRE(n_polys >= 0 && n_pairs >= 0, "a negative count");
    VKX_REQUIRE(ctx, "NULL argument");
    VKX_REQUIRE(n_polys > 0 || n_pairs == 0, "a pair index out of range");
    if (n_polys == 0) return VKX_OK;
    VKX_REQUIRE(polys_host && pts_host && counts && (pairs_host || n_pairs == 0), "NULL argument");
    std::vector<PlaneRec> planes((size_t)n_polys);
    long long total_pts = 0, words = 0;
    for (int i = 0; i < n_polys; i++) {
        const vkx_poly_overlap_rec &g = polys_host[i];
        VKX_REQUIRE(g.h >= 1 && g.w >= 1 && g.h <= kMaxSide && g.w <= kMaxSide, "a box side outside 1 .. 32767");
        VKX_REQUIRE(g.pts_cnt >= 1 && g.pts_off >= 0 && g.pts_off <= INT_MAX - g.pts_cnt,
                    "a polygon of fewer than 1 point, or a bad point range");
        // (so that window arithmetic on up + h and left + w stays inside an int)
        VKX_REQUIRE(g.up >= -(1 << 30) && g.up <= (1 << 30) && g.left >= -(1 << 30) && g.left <= (1 << 30), "a box beyond 2^30");
        total_pts += g.pts_cnt;
        planes[i] = PlaneRec{words, g.up, g.left, g.h, g.w};
        words += (long long)g.h * row_words(g.w);
    }
    VKX_REQUIRE((unsigned long long)words * 4 <= (unsigned long long)VKX_POLY_OVERLAP_MAX_SCRATCH,
                "the bit planes need more than VKX_POLY_OVERLAP_MAX_SCRATCH bytes of scratch: split the candidates");
    // the work items: large ones first (a workgroup each), then the small ones (16 a workgroup)
    const size_t n_work = (size_t)n_polys + (size_t)n_pairs;
    std::vector<WorkRec> work;
    std::vector<WorkRec> small;
    work.reserve(n_work);
    small.reserve(n_work);
    for (int i = 0; i < n_polys; i++) {
        const PlaneRec &p = planes[i];
        const WorkRec wk{i, -1, i, 0};
        ((long long)p.h * row_words(p.w) > kSmallElems ? work : small).push_back(wk);
    }
    for (int k = 0; k < n_pairs; k++) {
        const int c = pairs_host[2 * (size_t)k], a = pairs_host[2 * (size_t)k + 1];
        VKX_REQUIRE(c >= 0 && c < n_polys && a >= 0 && a < n_polys, "a pair index out of range");
        const PlaneRec &pc = planes[c], &pa = planes[a];
        const int up = std::max(pc.up, pa.up), down = std::min(pc.up + pc.h, pa.up + pa.h);
        const int left = std::max(pc.left, pa.left), right = std::min(pc.left + pc.w, pa.left + pa.w);
        long long elems = 0;
        if (up < down && left < right) elems = (long long)(down - up) * (((right - 1 - pc.left) >> 5) - ((left - pc.left) >> 5) + 1);
        const WorkRec wk{c, a, n_polys + k, 0};
        (elems > kSmallElems ? work : small).push_back(wk);
    }
    const int n_large = (int)work.size();
    work.insert(work.end(), small.begin(), small.end());
    VKX_REQUIRE(n_work < 0x3fffffff, "too many work items");
    // every polygon in box-relative coordinates (its points are self-relative already), its scanlines inside its box
    vkp::Raster<vkp::kPaintCross> raster;
    VKX_REQUIRE(raster.reserve(total_pts), "too many vertices");
    for (int i = 0; i < n_polys; i++) {
        const vkx_poly_overlap_rec &g = polys_host[i];
        VKX_REQUIRE(raster.add(pts_host + 2 * (size_t)g.pts_off, g.pts_cnt, 1, i, 0, g.h), "polygon outlines too long");
    }

    vkx_tables tab(ctx);             // behind the overflow flag's 256 bytes of ctx->ov_tables
    const size_t p_off = tab.add(sizeof(PlaneRec) * planes.size());
    const size_t w_off = tab.add(sizeof(WorkRec) * work.size());
    raster.layout(tab);
    int rc = vkx_scratch_reserve(ctx, &ctx->ov_tables, std::max(256 + vkx_align256(tab.bytes), (size_t)64 << 10));
    if (rc) return rc;
    const size_t bits_bytes = (size_t)words * 4;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->ov_bits, bits_bytes))) return rc;
    unsigned char *base = (unsigned char *)ctx->ov_tables.ptr;
    int *overflow = (int *)base;
    const PlaneRec *d_planes = (const PlaneRec *)(base + 256 + p_off);
    const WorkRec *d_work = (const WorkRec *)(base + 256 + w_off);
    unsigned *bits = (unsigned *)ctx->ov_bits.ptr;
    // The tables travel through the context's page-locked ring as ONE asynchronous copy: the call returns with its kernels
    // queued unless a polygon could overflow (vkp::Raster).
    vkx_device_guard guard(ctx);
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<PlaneRec>(p_off), planes.data(), sizeof(PlaneRec) * planes.size());
    memcpy(tab.at<WorkRec>(w_off), work.data(), sizeof(WorkRec) * work.size());
    raster.stage(tab);
    if ((rc = tab.copy_to(base + 256))) return rc;
    VKX_HIP(hipMemsetAsync(bits, 0, bits_bytes, ctx->stream));
    // (polygons that are all flat have no scanline item: the span launch stays, one idle workgroup, so that the launches of a
    //  call do not depend on its polygons)
    if ((rc = raster.launch(ctx, base + 256, overflow, BitRowSink{d_planes, bits}, "k_overlap_outline", "k_overlap_spans", true))) return rc;
    const unsigned blocks = (unsigned)n_large + vkx_blocks(small.size(), 16);
    { VKX_TIMED(ctx, "k_overlap_count"); k_overlap_count<<<blocks, 256, 0, ctx->stream>>>(d_planes, bits, d_work, (int)n_work, n_large, counts); }
    VKX_LAUNCH_CHECK();
    return raster.finish(ctx, overflow, "a polygon");
}

VKX_EXPORT int vkx_mask_overlap_counts_dev(vkx_ctx *ctx, const vkx_mask_overlap_rec *recs_host, int n_recs, int64_t *counts)
{
    VKX_REQUIRE(n_recs >= 0 && n_recs <= kMaxMaskRecs, "0 .. 65536 records");
    VKX_REQUIRE(ctx, "NULL argument");
    if (n_recs == 0) return VKX_OK;
    VKX_REQUIRE(recs_host && counts, "NULL argument");
    for (int i = 0; i < n_recs; i++) {
        const vkx_mask_overlap_rec &r = recs_host[i];
        VKX_REQUIRE(r.anchor && r.candidate, "NULL plane");
        VKX_REQUIRE(r.anchor_h >= 1 && r.anchor_w >= 1 && r.anchor_h <= kMaxSide && r.anchor_w <= kMaxSide && r.candidate_h >= 1 &&
                        r.candidate_w >= 1 && r.candidate_h <= kMaxSide && r.candidate_w <= kMaxSide,
                    "a box side outside 1 .. 32767");
        VKX_REQUIRE(r.anchor_up >= -(1 << 30) && r.anchor_up <= (1 << 30) && r.anchor_left >= -(1 << 30) && r.anchor_left <= (1 << 30) &&
                        r.candidate_up >= -(1 << 30) && r.candidate_up <= (1 << 30) && r.candidate_left >= -(1 << 30) &&
                        r.candidate_left <= (1 << 30),
                    "a box beyond 2^30");
        VKX_REQUIRE_PITCH(r.anchor_step, r.anchor_w, r.anchor_h);
        VKX_REQUIRE_PITCH(r.candidate_step, r.candidate_w, r.candidate_h);
        VKX_REQUIRE(!vkx_planes_overlap(counts, 1, 0, sizeof(int64_t) * 3 * (size_t)n_recs, r.anchor, r.anchor_h, r.anchor_step, (size_t)r.anchor_w) &&
                        !vkx_planes_overlap(counts, 1, 0, sizeof(int64_t) * 3 * (size_t)n_recs, r.candidate, r.candidate_h, r.candidate_step,
                                            (size_t)r.candidate_w),
                    "counts overlaps a plane");
    }
    vkx_tables tab(ctx);
    int rc = tab.take(sizeof(vkx_mask_overlap_rec) * (size_t)n_recs);
    if (rc) return rc;
    memcpy(tab.at<vkx_mask_overlap_rec>(0), recs_host, sizeof(vkx_mask_overlap_rec) * (size_t)n_recs);
    if ((rc = tab.copy_to(&ctx->ov_tables, (size_t)64 << 10))) return rc;
    { VKX_TIMED(ctx, "k_mask_overlap_count"); k_mask_overlap_count<<<n_recs, 256, 0, ctx->stream>>>((const vkx_mask_overlap_rec *)ctx->ov_tables.ptr, (long long *)counts); }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
