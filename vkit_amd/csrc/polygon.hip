// The polygon rasters of the C ABI on gfx950: cv.fillPoly(mask, [pts], 1) for one polygon of any vertex count
// (reference: PolygonInternals.np_mask, element/polygon.py:70-77; used by Polygon.fill_* and by the active mask
// of image-grid distortions, grid_rendering/interface.py:177-192) and the ordered paint of the polygons of a page.
//
// The raster is vkx_poly_raster.h's (vkp::k_outline, vkp::k_spans, the host-side vkp::Raster), shared with region_masks.hip.
// What is here: the two sinks -- a byte store of 1 for the single polygon, atomicMax of the paint order into an ownership raster
// for the paint --, the paint's resolve kernel and the entry points.
// Vertices are host data (a few to a few thousand points); the edge table is built on the host and staged.
#include "vkx_internal.h"
#include "vkx_host_stage.h"
#include <string.h>
#include "vkx_poly_raster.h"

namespace {

struct ByteSink {              // vkx_fill_poly_mask_u8_dev: mask[y][x] = 1 inside [h, w]
    uint8_t *mask;
    int h, w;
    ptrdiff_t stride;
    struct Row {
        uint8_t *p;
        int w;
        __device__ void operator()(int x) const { p[x] = 1; }
    };
    __device__ void pixel(const vkp::PolyEdge &, int x, int y) const
    {
        if ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) mask[(ptrdiff_t)y * stride + x] = 1;
    }
    __device__ Row row(const vkp::Item &item) const { return Row{mask + (ptrdiff_t)item.y * stride, (unsigned)item.y < (unsigned)h ? w : 0}; }
};

// ---- batched ordered paint: many polygons, later ones win ------------------------------------------------------
// Several label plane sets painted by one call live in bands of h rows of one ownership raster of `rows` rows: the target of a
// polygon is its band (its items are clipped to the band on the host, its outline here), its tag the 1-based paint order.
struct PaintSink {
    int *owner;
    int h, w, rows;
    struct Row {
        int *p;
        int w, order;
        __device__ void operator()(int x) const { atomicMax(&p[x], order); }
    };
    __device__ void pixel(const vkp::PolyEdge &e, int x, int y) const
    {
        if ((unsigned)x < (unsigned)w && (unsigned)(y - e.pad * h) < (unsigned)h) atomicMax(&owner[(size_t)y * w + x], e.poly);
    }
    __device__ Row row(const vkp::Item &item) const { return Row{owner + (size_t)item.y * w, (unsigned)item.y < (unsigned)rows ? w : 0, item.tag}; }
};

// FRESH: the output planes are uninitialised memory -- every pixel is written (0 outside every polygon), so the caller needs no
// memset of its own.  Either way the owner word is cleared as it is read: the raster is all zero again when the kernel is done and
// the next call needs no memset either (a page paints four label plane sets: 3 - 4 fill dispatches per call were 14 of its 98).
// blockIdx.z = the band of the raster = the plane set (vkx_paint_poly_sets_fresh_dev: the sets of a page in one call).
constexpr int kPaintSets = 8;
struct PaintOut {
    uint8_t *mask[kPaintSets];
    float *score[kPaintSets];
    ptrdiff_t mask_stride[kPaintSets], score_stride[kPaintSets];
    int value_off[kPaintSets];      // the set's first value in `values`
};

template <bool FRESH>
__global__ void __launch_bounds__(256) k_paint_resolve(int *__restrict__ owner_all, const float *__restrict__ values, PaintOut out, int h, int w)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int set = blockIdx.z;
    if (x >= w || y >= h) return;
    int *owner = owner_all + (size_t)set * h * w;
    uint8_t *mask = out.mask[set];
    float *score = out.score[set];
    const int o = owner[(size_t)y * w + x];
    if (o <= 0) {
        if (o < 0) owner[(size_t)y * w + x] = 0;
        if (FRESH) {
            if (mask) mask[(ptrdiff_t)y * out.mask_stride[set] + x] = 0;
            if (score) score[(ptrdiff_t)y * out.score_stride[set] + x] = 0.0f;
        }
        return;
    }
    owner[(size_t)y * w + x] = 0;
    if (mask) mask[(ptrdiff_t)y * out.mask_stride[set] + x] = 1;
    if (score) score[(ptrdiff_t)y * out.score_stride[set] + x] = values[out.value_off[set] + o - 1];
}

} // namespace

// The ordered paint of up to kPaintSets label plane sets of one shape in ONE call: set k's polygons are shifted into band k (rows
// [k h, (k + 1) h)) of one ownership raster and clipped to it, so one table copy and three kernels serve all of them (a page paints four
// sets -- text-line mask + heights, char mask, seal char mask, char heights: 16 dispatches as four calls, 4 as one).
static int paint_sets_dev(vkx_ctx *ctx, const vkx_paint_set *sets, int n_sets, int h, int w, bool fresh)
{
    VKX_REQUIRE(ctx && sets, "NULL argument");
    VKX_REQUIRE(n_sets >= 1 && n_sets <= kPaintSets, "1 .. 8 plane sets per call");
    VKX_REQUIRE(h > 0 && w > 0 && (long long)h * n_sets < 0x3fffffff, "bad shape");
    long long total_pts = 0, total_polys = 0;
    for (int k = 0; k < n_sets; k++) {
        const vkx_paint_set &S = sets[k];
        VKX_REQUIRE(S.n_polys >= 0 && (S.n_polys == 0 || (S.pts_host && S.poly_offsets_host)), "bad polygon list");
        VKX_REQUIRE(S.mask || S.score, "no output plane");
        VKX_REQUIRE_PITCH(S.mask_stride, w, S.mask ? h : 1);
        VKX_REQUIRE_PITCH(S.score_stride_el, w, S.score ? h : 1);
        VKX_REQUIRE(!S.score || S.values_host || S.n_polys == 0, "score output needs per-polygon values");
        if (S.n_polys) {
            VKX_REQUIRE(S.poly_offsets_host[S.n_polys] >= 0, "bad polygon offsets");
            total_pts += S.poly_offsets_host[S.n_polys];
            total_polys += S.n_polys;
        }
    }
    vkp::Raster<vkp::kPaintCross> raster;
    VKX_REQUIRE(raster.reserve(total_pts), "too many vertices");
    if (total_polys == 0 && !fresh) return VKX_OK;
    std::vector<float> values((size_t)total_polys);
    PaintOut out;
    memset(&out, 0, sizeof(out));
    bool any_values = false;
    size_t v_base = 0;
    for (int k = 0; k < n_sets; k++) {
        const vkx_paint_set &S = sets[k];
        out.mask[k] = S.mask; out.mask_stride[k] = S.mask_stride;
        out.score[k] = S.score; out.score_stride[k] = S.score_stride_el;
        out.value_off[k] = (int)v_base;
        if (S.n_polys == 0) continue;
        const int set_pts = S.poly_offsets_host[S.n_polys];
        const int y_off = k * h;            // the band: the set's vertices moved down by k h rows
        for (int p = 0; p < S.n_polys; p++) {
            const int b = S.poly_offsets_host[p], e = S.poly_offsets_host[p + 1];
            VKX_REQUIRE(b <= e && e <= set_pts, "bad polygon offsets");
            if (b == e) continue;
            VKX_REQUIRE(raster.add(S.pts_host + 2 * (size_t)b, e - b, p + 1, k, y_off, y_off + h, 0, y_off), "polygon outlines too long");
        }
        if (S.values_host) { memcpy(values.data() + v_base, S.values_host, sizeof(float) * (size_t)S.n_polys); any_values = true; }
        v_base += (size_t)S.n_polys;
    }
    vkx_tables tab(ctx);         // behind the overflow flag's 256 bytes of ctx->misc
    raster.layout(tab);
    const size_t v_off = tab.add(sizeof(float) * values.size());
    int rc = vkx_scratch_reserve(ctx, &ctx->misc, 256 + vkx_align256(tab.bytes));
    if (rc) return rc;
    // the ownership raster is the paint's own block: zero at rest (k_paint_resolve clears what it reads), memset only when it grows
    const size_t owner_bytes = (size_t)h * w * 4 * (size_t)n_sets;
    if (owner_bytes > ctx->paint_owner.cap) ctx->paint_owner_zeroed = 0;
    rc = vkx_scratch_reserve(ctx, &ctx->paint_owner, owner_bytes);
    if (rc) return rc;
    unsigned char *misc = (unsigned char *)ctx->misc.ptr;
    int *overflow = (int *)misc;
    float *d_values = (float *)(misc + 256 + v_off);
    int *owner = (int *)ctx->paint_owner.ptr;
    // The edge / item / value tables travel through the context's page-locked ring as ONE asynchronous copy: the call returns
    // with its kernels queued (a page paints four label planes: two stream synchronisations and a flag read-back per call were
    // 0.45 ms of a 2.2 ms page) unless a polygon could overflow (vkp::Raster).
    vkx_device_guard guard(ctx);
    if (tab.bytes) {
        if ((rc = tab.take())) return rc;
        raster.stage(tab);
        if (!values.empty()) memcpy(tab.at<float>(v_off), values.data(), sizeof(float) * values.size());
        if ((rc = tab.copy_to(misc + 256))) return rc;
    }
    if (ctx->paint_owner_zeroed < owner_bytes) VKX_HIP(hipMemsetAsync(owner, 0, ctx->paint_owner.cap, ctx->stream));
    ctx->paint_owner_zeroed = 0;          // dirty until the resolve kernel of THIS call has been queued (an error exit in between re-zeroes next time)
    if ((rc = raster.launch(ctx, misc + 256, overflow, PaintSink{owner, h, w, h * n_sets}, "k_paint_outline", "k_paint_spans", false))) return rc;
    {
        dim3 grid(vkx_blocks(w, 64), vkx_blocks(h, 4), n_sets);
        VKX_TIMED(ctx, "k_paint_resolve");
        if (fresh) k_paint_resolve<true><<<grid, 256, 0, ctx->stream>>>(owner, any_values ? d_values : nullptr, out, h, w);
        else k_paint_resolve<false><<<grid, 256, 0, ctx->stream>>>(owner, any_values ? d_values : nullptr, out, h, w);
        VKX_LAUNCH_CHECK();
        ctx->paint_owner_zeroed = ctx->paint_owner.cap;
    }
    return raster.finish(ctx, overflow, "a polygon");
}

static int paint_polys_dev(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                           const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                           ptrdiff_t score_stride_el, int h, int w, bool fresh)
{
    VKX_REQUIRE(ctx && (n_polys == 0 || (pts_host && poly_offsets_host)), "NULL argument");
    VKX_REQUIRE(n_polys >= 0 && h > 0 && w > 0, "bad shape");
    vkx_paint_set S;
    S.pts_host = pts_host; S.poly_offsets_host = poly_offsets_host; S.n_polys = n_polys; S.values_host = values_host;
    S.mask = mask; S.mask_stride = mask_stride; S.score = score; S.score_stride_el = score_stride_el;
    return paint_sets_dev(ctx, &S, 1, h, w, fresh);
}

VKX_EXPORT int vkx_paint_poly_sets_fresh_dev(vkx_ctx *ctx, const vkx_paint_set *sets, int n_sets, int h, int w)
{
    return paint_sets_dev(ctx, sets, n_sets, h, w, true);
}

VKX_EXPORT int vkx_paint_polys_dev(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                                   const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                                   ptrdiff_t score_stride_el, int h, int w)
{
    return paint_polys_dev(ctx, pts_host, poly_offsets_host, n_polys, values_host, mask, mask_stride, score, score_stride_el, h, w, false);
}

VKX_EXPORT int vkx_paint_polys_fresh_dev(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                                         const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                                         ptrdiff_t score_stride_el, int h, int w)
{
    return paint_polys_dev(ctx, pts_host, poly_offsets_host, n_polys, values_host, mask, mask_stride, score, score_stride_el, h, w, true);
}

// Host planes: mask / score are updated in place (read, painted, written back).
VKX_EXPORT int vkx_paint_polys(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                               const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                               ptrdiff_t score_stride_el, int h, int w)
{
    VKX_REQUIRE(ctx && (mask || score), "NULL argument");
    VKX_REQUIRE(h > 0 && w > 0, "bad shape");
    VKX_REQUIRE_PITCH(mask_stride, w, mask ? h : 1);
    VKX_REQUIRE_PITCH(score_stride_el, w, score ? h : 1);
    const size_t mbytes = mask ? vkx_align256((size_t)h * w) : 0;
    const size_t sbytes = score ? (size_t)h * w * 4 : 0;
    int rc = vkx_scratch_reserve(ctx, &ctx->stage[1], mbytes + sbytes);
    if (rc) return rc;
    uint8_t *d_mask = mask ? (uint8_t *)ctx->stage[1].ptr : nullptr;
    float *d_score = score ? (float *)((unsigned char *)ctx->stage[1].ptr + mbytes) : nullptr;
    if (mask)
        VKX_HIP(vkx_copy_plane(d_mask, (size_t)w, mask, (size_t)mask_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    if (score)
        VKX_HIP(vkx_copy_plane(d_score, (size_t)w * 4, score, (size_t)score_stride_el * 4, (size_t)w * 4, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    rc = vkx_paint_polys_dev(ctx, pts_host, poly_offsets_host, n_polys, values_host, d_mask, w, d_score, w, h, w);
    if (rc) return rc;
    if (mask)
        VKX_HIP(vkx_copy_plane(mask, (size_t)mask_stride, d_mask, (size_t)w, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, ctx->stream));
    if (score)
        VKX_HIP(vkx_copy_plane(score, (size_t)score_stride_el * 4, d_score, (size_t)w * 4, (size_t)w * 4, (size_t)h, hipMemcpyDeviceToHost, ctx->stream));
    VKX_HIP(hipStreamSynchronize(ctx->stream));
    return VKX_OK;
}

VKX_EXPORT int vkx_fill_poly_mask_u8_dev(vkx_ctx *ctx, const int32_t *pts_host, int npts, uint8_t *mask, int h, int w,
                                         ptrdiff_t stride)
{
    VKX_REQUIRE(ctx && pts_host && mask, "NULL argument");
    VKX_REQUIRE(npts > 0 && h > 0 && w > 0, "bad shape");
    VKX_REQUIRE_PITCH(stride, w, h);
    for (int i = 0; i < npts; i++) {
        const int xb = pts_host[2 * i], yb = pts_host[2 * i + 1];
        VKX_REQUIRE(xb >= 0 && xb < w && yb >= 0 && yb < h, "polygon vertex outside the mask");
    }
    vkp::Raster<vkp::kPolyCross> raster;
    VKX_REQUIRE(raster.reserve(npts), "too many vertices");
    VKX_REQUIRE(raster.add(pts_host, npts, 0, 0), "polygon outline too long");
    vkx_tables tab(ctx);         // behind the overflow flag's 256 bytes of ctx->misc
    raster.layout(tab);
    int rc = vkx_scratch_reserve(ctx, &ctx->misc, 256 + vkx_align256(tab.bytes));
    if (rc) return rc;
    unsigned char *misc = (unsigned char *)ctx->misc.ptr;
    int *overflow = (int *)misc;
    vkx_device_guard guard(ctx);
    if ((rc = tab.take())) return rc;
    raster.stage(tab);
    if ((rc = tab.copy_to(misc + 256))) return rc;
    if ((rc = raster.launch(ctx, misc + 256, overflow, ByteSink{mask, h, w, stride}, "k_poly_outline", "k_poly_spans", false))) return rc;
    return raster.finish(ctx, overflow, "polygon");
}

// Host-memory variant: zero-initialised mask of shape [h, w] with the polygon set to 1.
VKX_EXPORT int vkx_fill_poly_mask_u8(vkx_ctx *ctx, const int32_t *pts_host, int npts, uint8_t *mask, int h, int w,
                                     ptrdiff_t stride)
{
    VKX_REQUIRE(ctx && pts_host && mask, "NULL argument");
    VKX_REQUIRE(npts > 0 && h > 0 && w > 0, "bad shape");
    auto m = vkx_out(mask, h, w, 1, stride);
    return vkx_host_run(ctx, {&m}, [&] {
        vkx_device_guard guard(ctx);
        VKX_HIP(hipMemsetAsync(m.dev(), 0, (size_t)h * w, ctx->stream));
        return vkx_fill_poly_mask_u8_dev(ctx, pts_host, npts, m.dev(), h, w, m.pitch);
    });
}
