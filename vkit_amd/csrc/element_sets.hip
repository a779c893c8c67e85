// The set-operation mask of a list of elements on gfx950 (reference: element/mask.py:126-244 Mask._from_np_active_count and
// Mask.from_boxes / from_polygons / from_masks / from_score_maps; consumed by generate_fill_by_*_mask and the fill_by_* families of
// element/image.py:371-665, element/mask.py:283-410 and element/score_map.py:315-520).
//
// The reference adds 1 to an int32 count plane under every element of the list, one numpy pass an element, and thresholds the
// count: UNION > 0, DISTINCT == 1, INTERSECT > 1.  The three predicates only ask whether a pixel was touched by no entry, by one
// or by more than one, so no counter is kept: two int planes hold, per pixel, the largest (entry index + 1) and the largest
// (INT_MAX - entry index) that touched it, both by atomicMax on zeroed memory.  Untouched: 0; one entry: the two name the same
// index; more than one: they differ.  The maximum of a set does not depend on the order its members arrive in, and an entry that
// touches a pixel twice (a polygon's outline and its spans overlap) leaves what it left the first time; an entry listed twice has
// two indices and counts twice, as it does in the reference.  At most FOUR launches whatever the length of the list:
//   k_set_outline   vkp::k_outline over every polygon: the LINE_8 outline pixels
//   k_set_spans     vkp::k_spans: one wave per (polygon, scanline), the even-odd spans
//   k_set_planes    one lane per pixel of the window of every box, mask and score map
//   k_set_resolve   one lane per pixel of the plane: dst = the mode's predicate (every byte written); then one lane per pixel of
//                   every window: the entry's own active raster, on request ANDed with the predicate
// The raster is vkx_poly_raster.h's (pixel for pixel vkx_fill_poly_mask_u8's); what is here is its sink, SetSink.  Small,
// latency-bound kernels; vector atomics and plain vector stores only.
#include "vkx_internal.h"
#include "vkx_host_stage.h"
#include "vkx_poly_raster.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int kMaxElems = 1 << 16;
constexpr int kMaxSide = 32767;

struct SetRec {
    const void *plane;
    long long plane_step, window_off;
    int kind, up, left, h, w;
    int plane_tile, win_tile;        // prefixes of the 256-pixel tiles of k_set_planes / of the window half of k_set_resolve
};

__device__ __forceinline__ void touch(int *__restrict__ hi, int *__restrict__ lo, size_t p, int e)
{
    atomicMax(&hi[p], e + 1);
    atomicMax(&lo[p], INT_MAX - e);
}

// 0: no entry, 1: one entry, 2: more than one
__device__ __forceinline__ int count_class(const int *__restrict__ hi, const int *__restrict__ lo, size_t p)
{
    const int a = hi[p];
    if (a == 0) return 0;
    return INT_MAX - lo[p] == a - 1 ? 1 : 2;
}

__device__ __forceinline__ bool holds(int mode, int c) { return mode == 0 ? c > 0 : (mode == 1 ? c == 1 : c == 2); }

// is pixel (y, x) of the window of a box, mask or score map active?
__device__ __forceinline__ bool plane_active(const SetRec &r, int y, int x)
{
    if (r.kind == VKX_SET_BOX) return true;
    const unsigned char *row = (const unsigned char *)r.plane + (ptrdiff_t)y * r.plane_step;
    if (r.kind == VKX_SET_MASK_U8) return row[x] > 0;
    return ((const float *)row)[x] > 0.0f;
}

// The target of a polygon is its entry; a pixel outside the entry's window is dropped (the host refuses such a polygon).
struct SetSink {
    const SetRec *recs;
    int *hi, *lo;
    uint8_t *windows;
    int h, w;
    struct Row {
        int *hi, *lo;
        uint8_t *win;
        int w, left, rw, e;
        __device__ void operator()(int x) const
        {
            if ((unsigned)(x - left) >= (unsigned)rw) return;
            touch(hi, lo, (size_t)x, e);
            if (win) win[x - left] = 1;
        }
    };
    __device__ void pixel(const vkp::PolyEdge &e, int x, int y) const
    {
        const SetRec r = recs[e.pad];
        if ((unsigned)(x - r.left) >= (unsigned)r.w || (unsigned)(y - r.up) >= (unsigned)r.h) return;
        touch(hi, lo, (size_t)y * w + x, e.pad);
        if (windows) windows[r.window_off + (long long)(y - r.up) * r.w + (x - r.left)] = 1;
    }
    __device__ Row row(const vkp::Item &item) const
    {
        const SetRec r = recs[item.target];
        const bool inside = (unsigned)(item.y - r.up) < (unsigned)r.h;
        const size_t base = inside ? (size_t)item.y * w : 0;
        return Row{hi + base, lo + base, windows && inside ? windows + r.window_off + (long long)(item.y - r.up) * r.w : nullptr,
                   inside ? w : 0, r.left, r.w, item.target};
    }
};

// grid: the 256-pixel tiles of the windows of the boxes, masks and score maps
__global__ void __launch_bounds__(256) k_set_planes(const SetRec *__restrict__ recs, int n, int *__restrict__ hi, int *__restrict__ lo, int w)
{
    const int t = blockIdx.x;
    const int e = vkd::last_at_most(n, t, [&](int i) { return recs[i].plane_tile; });
    const SetRec r = recs[e];
    const int idx = (t - r.plane_tile) * 256 + threadIdx.x;
    if (r.kind == VKX_SET_POLYGON || idx >= r.h * r.w) return;
    const int y = idx / r.w, x = idx - y * r.w;
    if (plane_active(r, y, x)) touch(hi, lo, (size_t)(r.up + y) * w + r.left + x, e);
}

// grid: plane_tiles tiles of the plane, then the tiles of the windows (none without `windows`)
__global__ void __launch_bounds__(256) k_set_resolve(const SetRec *__restrict__ recs, int n, const int *__restrict__ hi,
                                                     const int *__restrict__ lo, int mode, int gated, int h, int w, int plane_tiles,
                                                     uint8_t *__restrict__ dst, ptrdiff_t dst_step, uint8_t *__restrict__ windows)
{
    if ((int)blockIdx.x < plane_tiles) {
        const int p = blockIdx.x * 256 + threadIdx.x;
        if (p >= h * w) return;
        const int y = p / w, x = p - y * w;
        dst[(ptrdiff_t)y * dst_step + x] = holds(mode, count_class(hi, lo, (size_t)p)) ? 1 : 0;
        return;
    }
    const int t = blockIdx.x - plane_tiles;
    const int e = vkd::last_at_most(n, t, [&](int i) { return recs[i].win_tile; });
    const SetRec r = recs[e];
    const int idx = (t - r.win_tile) * 256 + threadIdx.x;
    if (idx >= r.h * r.w) return;
    const int y = idx / r.w, x = idx - y * r.w;
    uint8_t *out = windows + r.window_off + idx;
    bool own = r.kind == VKX_SET_POLYGON ? *out != 0 : plane_active(r, y, x);
    if (gated) own = own && holds(mode, count_class(hi, lo, (size_t)(r.up + y) * w + r.left + x));
    if (r.kind != VKX_SET_POLYGON || gated) *out = own ? 1 : 0;
}

int check_call(const vkx_set_elem *elems, int n, const int32_t *pts, int n_pts, int mode, int h, int w, const uint8_t *dst,
               ptrdiff_t dst_step, const uint8_t *windows, size_t window_bytes, bool device_planes)
{
    VKX_REQUIRE(n >= 0 && n <= kMaxElems, "0 .. 65536 elements");
    VKX_REQUIRE(dst && (n == 0 || elems), "NULL argument");
    VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "a plane side outside 1 .. 32767");
    VKX_REQUIRE((mode & ~VKX_SET_WINDOWS_GATED) >= 0 && (mode & ~VKX_SET_WINDOWS_GATED) <= 2, "mode outside UNION, DISTINCT, INTERSECT");
    VKX_REQUIRE(n_pts >= 0, "bad point count");
    VKX_REQUIRE_PITCH(dst_step, w, h);
    for (int i = 0; i < n; i++) {
        const vkx_set_elem &g = elems[i];
        VKX_REQUIRE(g.kind >= VKX_SET_BOX && g.kind <= VKX_SET_SCORE_F32, "unknown element kind");
        VKX_REQUIRE(g.h >= 1 && g.w >= 1 && g.up >= 0 && g.left >= 0 && g.up <= h - g.h && g.left <= w - g.w,
                    "an element window outside the plane");
        const long long area = (long long)g.h * g.w;
        if (windows)
            VKX_REQUIRE(g.window_off >= 0 && (unsigned long long)(g.window_off + area) <= window_bytes, "window_bytes too small for an element window");
        if (g.kind == VKX_SET_POLYGON) {
            VKX_REQUIRE(pts && g.pts_cnt >= 1 && g.pts_off >= 0 && g.pts_off <= n_pts - g.pts_cnt, "a polygon of fewer than 1 point, or a bad point range");
            for (int j = g.pts_off; j < g.pts_off + g.pts_cnt; j++) {
                const int x = pts[2 * (size_t)j], y = pts[2 * (size_t)j + 1];
                VKX_REQUIRE(x >= g.left && x - g.left < g.w && y >= g.up && y - g.up < g.h, "a polygon vertex outside its window");
            }
        } else if (g.kind != VKX_SET_BOX) {
            const size_t esz = g.kind == VKX_SET_SCORE_F32 ? 4 : 1;
            VKX_REQUIRE(g.plane, "a mask or score-map element without its plane");
            VKX_REQUIRE_PITCH(g.plane_step, (ptrdiff_t)(g.w * esz), g.h);
            if (device_planes) {
                VKX_REQUIRE(!vkx_planes_overlap(g.plane, g.h, (ptrdiff_t)g.plane_step, g.w * esz, dst, h, dst_step, (size_t)w), "an element plane overlaps dst");
                VKX_REQUIRE(!windows || !vkx_planes_overlap(g.plane, g.h, (ptrdiff_t)g.plane_step, g.w * esz, windows, 1, 0, window_bytes),
                            "an element plane overlaps the windows");
            }
        }
    }
    VKX_REQUIRE(!windows || !vkx_planes_overlap(dst, h, dst_step, (size_t)w, windows, 1, 0, window_bytes), "dst overlaps the windows");
    return VKX_OK;
}

}  // namespace

VKX_EXPORT int vkx_set_mask_dev(vkx_ctx *ctx, const vkx_set_elem *elems_host, int n, const int32_t *pts_host, int n_pts, int mode,
                                int h, int w, uint8_t *dst, ptrdiff_t dst_step, uint8_t *windows, size_t window_bytes)
{
    VKX_REQUIRE(ctx, "NULL argument");
    int rc = check_call(elems_host, n, pts_host, n_pts, mode, h, w, dst, dst_step, windows, window_bytes, true);
    if (rc) return rc;
    vkx_device_guard guard(ctx);
    if (n == 0) {        // the count plane of an empty list is zero: no pixel holds any predicate
        VKX_HIP(hipMemset2DAsync(dst, h > 1 ? (size_t)dst_step : (size_t)w, 0, (size_t)w, (size_t)h, ctx->stream));
        return VKX_OK;
    }
    const int gated = (mode & VKX_SET_WINDOWS_GATED) ? 1 : 0;
    mode &= ~VKX_SET_WINDOWS_GATED;
    std::vector<SetRec> recs((size_t)n);
    long long total_pts = 0, plane_tiles = 0, win_tiles = 0, poly_lo = LLONG_MAX, poly_hi = 0;
    for (int i = 0; i < n; i++) {
        const vkx_set_elem &g = elems_host[i];
        const long long area = (long long)g.h * g.w, tiles = (area + 255) / 256;
        recs[i] = SetRec{g.plane, g.plane_step, g.window_off, g.kind, g.up, g.left, g.h, g.w, (int)plane_tiles, (int)win_tiles};
        if (g.kind == VKX_SET_POLYGON) {
            total_pts += g.pts_cnt;
            poly_lo = std::min(poly_lo, (long long)g.window_off);
            poly_hi = std::max(poly_hi, g.window_off + area);
        } else {
            plane_tiles += tiles;
        }
        if (windows) win_tiles += tiles;
        VKX_REQUIRE(plane_tiles < 0x3fffffff && win_tiles < 0x3fffffff, "element windows too large in total");
    }
    vkp::Raster<vkp::kPaintCross> raster;
    VKX_REQUIRE(raster.reserve(total_pts), "too many vertices");
    for (int i = 0; i < n; i++) {
        const vkx_set_elem &g = elems_host[i];
        if (g.kind == VKX_SET_POLYGON) VKX_REQUIRE(raster.add(pts_host + 2 * (size_t)g.pts_off, g.pts_cnt, 0, i), "polygon outlines too long");
    }

    vkx_tables tab(ctx);             // behind the overflow flag's 256 bytes of ctx->set_tables
    const size_t r_off = tab.add(sizeof(SetRec) * recs.size());
    raster.layout(tab);
    if ((rc = vkx_scratch_reserve(ctx, &ctx->set_tables, std::max(256 + vkx_align256(tab.bytes), (size_t)64 << 10)))) return rc;
    const size_t plane_elems = (size_t)h * w;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->set_planes, plane_elems * 2 * sizeof(int)))) return rc;
    unsigned char *base = (unsigned char *)ctx->set_tables.ptr;
    int *overflow = (int *)base;
    const SetRec *d_recs = (const SetRec *)(base + 256 + r_off);
    int *hi = (int *)ctx->set_planes.ptr, *lo = hi + plane_elems;
    // The tables travel through the context's page-locked ring as ONE asynchronous copy: the call returns with its kernels queued
    // unless a polygon could overflow (vkp::Raster).
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<SetRec>(r_off), recs.data(), sizeof(SetRec) * recs.size());
    raster.stage(tab);
    if ((rc = tab.copy_to(base + 256))) return rc;
    VKX_HIP(hipMemsetAsync(hi, 0, plane_elems * 2 * sizeof(int), ctx->stream));
    // (a polygon's window starts from zero: its raster stores only the 1s)
    if (windows && poly_hi > poly_lo) VKX_HIP(hipMemsetAsync(windows + poly_lo, 0, (size_t)(poly_hi - poly_lo), ctx->stream));
    if ((rc = raster.launch(ctx, base + 256, overflow, SetSink{d_recs, hi, lo, windows, h, w}, "k_set_outline", "k_set_spans", false))) return rc;
    if (plane_tiles > 0) {
        { VKX_TIMED(ctx, "k_set_planes"); k_set_planes<<<(unsigned)plane_tiles, 256, 0, ctx->stream>>>(d_recs, n, hi, lo, w); }
        VKX_LAUNCH_CHECK();
    }
    const int dst_tiles = (int)vkx_blocks(plane_elems, 256);
    { VKX_TIMED(ctx, "k_set_resolve"); k_set_resolve<<<(unsigned)(dst_tiles + win_tiles), 256, 0, ctx->stream>>>(d_recs, n, hi, lo, mode, gated, h, w, dst_tiles, dst, dst_step, windows); }
    VKX_LAUNCH_CHECK();
    return raster.finish(ctx, overflow, "a polygon");
}

// Host planes: the element planes, dst and the windows are host memory; dst and the windows are overwritten.
VKX_EXPORT int vkx_set_mask(vkx_ctx *ctx, const vkx_set_elem *elems_host, int n, const int32_t *pts_host, int n_pts, int mode, int h,
                            int w, uint8_t *dst, ptrdiff_t dst_step, uint8_t *windows, size_t window_bytes)
{
    VKX_REQUIRE(ctx, "NULL argument");
    int rc = check_call(elems_host, n, pts_host, n_pts, mode, h, w, dst, dst_step, windows, window_bytes, false);
    if (rc) return rc;
    std::vector<vkx_set_elem> elems(elems_host, elems_host + n);
    std::vector<vkx_host_plane<uint8_t>> planes;
    planes.reserve((size_t)n + 2);
    planes.push_back(vkx_out(dst, h, (size_t)w, 1, dst_step));
    planes.push_back(vkx_out(windows, 1, windows ? window_bytes : 0, 1, 0));
    for (int i = 0; i < n; i++) {
        const vkx_set_elem &g = elems[i];
        if (g.kind != VKX_SET_MASK_U8 && g.kind != VKX_SET_SCORE_F32) continue;
        planes.push_back(vkx_in((const uint8_t *)g.plane, g.h, (size_t)g.w * (g.kind == VKX_SET_SCORE_F32 ? 4 : 1), 1, (ptrdiff_t)g.plane_step));
    }
    std::vector<vkx_host_plane_raw *> list;
    for (auto &p : planes) list.push_back(&p);
    return vkx_host_run(ctx, list.data(), list.size(), [&] {
        size_t k = 2;
        for (int i = 0; i < n; i++) {
            vkx_set_elem &g = elems[i];
            if (g.kind != VKX_SET_MASK_U8 && g.kind != VKX_SET_SCORE_F32) continue;
            g.plane = planes[k].dev();
            g.plane_step = planes[k].pitch;
            k++;
        }
        vkx_device_guard guard(ctx);
        if (windows) VKX_HIP(hipMemsetAsync(planes[1].dev(), 0, window_bytes, ctx->stream));     // (the bytes between the windows travel back too)
        return vkx_set_mask_dev(ctx, elems.data(), n, pts_host, n_pts, mode, h, w, planes[0].dev(), planes[0].pitch, planes[1].dev(), window_bytes);
    });
}
