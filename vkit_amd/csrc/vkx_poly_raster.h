// The cv::fillPoly raster (CollectPolyEdges + FillEdgeCollection), stated once: the LINE_8 outline walked from the left end of
// every edge, then the even-odd spans [ceil(xa), floor(xb)] over the 16.16 crossings of the half-open edges (y0 <= y < y1).
//   make_edge / build_edges   the edge record, on the host (contours of any length) or on the device (char_heatmap.hip's quads)
//   k_outline<Sink>           one lane per (edge, major step): the pixel of that step
//   k_spans<Sink, kCross>     one wave per (polygon, scanline): up to kCross crossings ranked in LDS, the spans filled lane-parallel
//   quad_covers               both in closed form for one pixel of a quad
//   Raster                    the host side of a call: contours -> edge and item tables -> the two launches -> the overflow flag
// What differs between the consumers is where a pixel goes: a Sink is a small device functor that owns the clip and the store.
//   sink.pixel(edge, x, y)    an outline pixel
//   sink.row(item)            the scanline of an item: `w` (pixels [0, w) of it are stored; 0: none) and operator()(x), the store
// The sinks live with their callers (polygon.hip: ownership paint, byte mask; region_masks.hip: bit planes).
#pragma once
#include "vkx_internal.h"
#include "vkx_cell.h"

#include <algorithm>
#include <cstring>

namespace vkp {

struct Edge {                  // one polygon edge, vertex a -> vertex b
    int lx, ly, dmaj, dmin;    // Bresenham from the left end (cv::LineIterator)
    int sy, ymajor;
    int y0, y1;                // scanline range of the edge (y0 == y1: horizontal, not in the edge table)
    long long x0_fix, dx_fix;  // 16.16 x at y0, dx per scanline
};

struct PolyEdge : Edge {       // ... in the edge table of a batch
    int step_base;             // prefix of (dmaj + 1) over the edges
    int poly, pad;             // the tag and the target of its polygon (Raster::add)
};

struct Item {                  // one (polygon, scanline) pair
    int edge_begin, edge_end;  // the polygon's edges
    int y;
    int target, tag;           // where the polygon goes and what it stores, as its sink reads them
};

__host__ __device__ inline Edge make_edge(int xa, int ya, int xb, int yb)
{
    Edge e;
    const bool swap = xb < xa;
    const int lx = swap ? xb : xa, ly = swap ? yb : ya, rx = swap ? xa : xb, ry = swap ? ya : yb;
    const int dx = rx - lx, dy = ry - ly, ady = dy < 0 ? -dy : dy;
    e.lx = lx; e.ly = ly; e.sy = dy < 0 ? -1 : 1;
    e.ymajor = ady > dx;
    e.dmaj = e.ymajor ? ady : dx;
    e.dmin = e.ymajor ? dx : ady;
    e.y0 = ya < yb ? ya : yb; e.y1 = ya < yb ? yb : ya;
    if (ya != yb) {
        const long long fa = (long long)xa * 65536, fb = (long long)xb * 65536;     // (a shift of a negative x is undefined before C++20)
        e.dx_fix = (fb - fa) / (long long)(yb - ya);
        e.x0_fix = ya < yb ? fa : fb;
    } else {
        e.dx_fix = 0; e.x0_fix = 0;
    }
    return e;
}

// Edge table of one closed contour, its vertices moved by (dx, dy); ymin / ymax: the scanline range of its non-horizontal edges.
static inline void build_edges(const int32_t *pts, int npts, int dx, int dy, int poly, int pad, PolyEdge *edges, long long *steps,
                               int *ymin, int *ymax)
{
    for (int i = 0; i < npts; i++) {
        const int a = (i + npts - 1) % npts;
        PolyEdge &e = edges[i];
        static_cast<Edge &>(e) = make_edge(pts[2 * a] + dx, pts[2 * a + 1] + dy, pts[2 * i] + dx, pts[2 * i + 1] + dy);
        e.step_base = (int)*steps;
        *steps += e.dmaj + 1;
        e.poly = poly; e.pad = pad;
        if (e.y0 != e.y1) { *ymin = std::min(*ymin, e.y0); *ymax = std::max(*ymax, e.y1); }
    }
}

// the edge that outline step t belongs to (step_base is a prefix sum), and the pixel of that step
__device__ __forceinline__ PolyEdge edge_of_step(const PolyEdge *__restrict__ edges, int nedges, int t)
{
    return edges[vkd::last_at_most(nedges, t, [&](int i) { return edges[i].step_base; })];
}

__device__ __forceinline__ void edge_pixel(const PolyEdge &e, int t, int &x, int &y)
{
    const int k = t - e.step_base;
    const int m = vkc::bres_minor(k, e.dmaj, e.dmin);
    x = e.ymajor ? e.lx + m : e.lx + k;
    y = e.ymajor ? e.ly + e.sy * k : e.ly + e.sy * m;
}

// One wave, one (polygon, scanline), in two steps that the workgroup's waves take together (each ends in __syncthreads).  xs /
// sorted: kCross words of LDS each and `count` one word, all the wave's own; `count` is zeroed by the caller before a barrier.
// wave_crossings: lanes test the polygon's edges [edge_begin, edge_end) and collect the 16.16 crossings of the half-open edges
// (y0 <= y < y1) in xs; returns their number, which may exceed the kCross that were kept (the caller's overflow).
template <int kCross>
__device__ __forceinline__ int wave_crossings(const PolyEdge *__restrict__ edges, int edge_begin, int edge_end, int y, long long *xs,
                                              int *count, int lane)
{
    for (int i = edge_begin + lane; i < edge_end; i += 64) {
        const PolyEdge &e = edges[i];
        if (e.y0 != e.y1 && e.y0 <= y && y < e.y1) {
            const int slot = atomicAdd(count, 1);
            if (slot < kCross) xs[slot] = e.x0_fix + (long long)(y - e.y0) * e.dx_fix;
        }
    }
    __syncthreads();
    return *count;
}

// wave_rank: the n <= kCross crossings ranked by counting into `sorted` (no sort loop: rank = number of crossings that
// precede it; the tie-break on the slot keeps the ranking a permutation).  A lane ranks slots lane, lane + 64, ...: one pass
// at kCross == 64.
template <int kCross>
__device__ __forceinline__ void wave_rank(const long long *xs, long long *sorted, int n, int lane)
{
    for (int base = 0; base < kCross; base += 64) {
        const int i = base + lane;
        if (i < n) {
            const long long v = xs[i];
            int rank = 0;
            for (int j = 0; j < n; j++) {
                const long long u = xs[j];
                rank += (u < v) || (u == v && j < i);
            }
            sorted[rank] = v;
        }
    }
    __syncthreads();
}

// the even-odd span a of the sorted crossings, clipped to [0, w): pixels [x1, x2]
__device__ __forceinline__ void span_of(const long long *sorted, int a, int w, long long &x1, long long &x2)
{
    x1 = (sorted[a] + 65535) >> 16;
    x2 = sorted[a + 1] >> 16;
    if (x1 < 0) x1 = 0;
    if (x2 >= w) x2 = w - 1;
}

template <class Sink>
__global__ void __launch_bounds__(256) k_outline(const PolyEdge *__restrict__ edges, int nedges, int total_steps, Sink sink)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total_steps) return;
    const PolyEdge e = edge_of_step(edges, nedges, t);
    int x, y;
    edge_pixel(e, t, x, y);
    sink.pixel(e, x, y);
}

// a polygon with more than kCross crossings on a scanline sets *overflow and paints no span of that scanline
template <class Sink, int kCross>
__global__ void __launch_bounds__(256) k_spans(const PolyEdge *__restrict__ edges, const Item *__restrict__ items, int n_items,
                                               Sink sink, int *__restrict__ overflow)
{
    __shared__ long long xs_all[4][kCross];
    __shared__ long long sorted_all[4][kCross];
    __shared__ int count_all[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int it = blockIdx.x * 4 + wave;
    const long long *sorted = sorted_all[wave];
    if (lane == 0) count_all[wave] = 0;
    __syncthreads();
    const bool live = it < n_items;
    Item item = {0, 0, 0, 0, 0};
    if (live) item = items[it];
    int n = wave_crossings<kCross>(edges, item.edge_begin, item.edge_end, item.y, xs_all[wave], &count_all[wave], lane);
    if (n > kCross) {
        if (lane == 0) atomicExch(overflow, 1);
        n = 0;
    }
    wave_rank<kCross>(xs_all[wave], sorted_all[wave], n, lane);
    if (!live) return;
    const auto row = sink.row(item);
    if (row.w <= 0) return;
    for (int a = 0; a + 1 < n; a += 2) {
        long long x1, x2;
        span_of(sorted, a, row.w, x1, x2);
        for (long long x = x1 + lane; x <= x2; x += 64) row((int)x);
    }
}

// cv.fillPoly(zeros(bh, bw), [quad], 1) at (x, y), as the oracle's closed form (vko_fill_poly_closed_form): inside an even-odd
// span of the row's crossings (at most 4 for a quad), or on the LINE_8 outline of an edge.
__device__ __forceinline__ bool quad_covers(const Edge (&E)[4], int x, int y)
{
    long long xs[4];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const bool hit = E[i].y0 != E[i].y1 && E[i].y0 <= y && y < E[i].y1;
        xs[i] = hit ? E[i].x0_fix + (long long)(y - E[i].y0) * E[i].dx_fix : LLONG_MAX;
        n += hit;
    }
    // sort 4 (unused slots hold LLONG_MAX and sort last)
#define VKX_CX(a, b) { const long long lo = xs[a] < xs[b] ? xs[a] : xs[b], hi = xs[a] < xs[b] ? xs[b] : xs[a]; xs[a] = lo; xs[b] = hi; }
    VKX_CX(0, 1) VKX_CX(2, 3) VKX_CX(0, 2) VKX_CX(1, 3) VKX_CX(1, 2)
#undef VKX_CX
    const long long X = x;
    if (n >= 2 && ((xs[0] + 65535) >> 16) <= X && X <= (xs[1] >> 16)) return true;
    if (n >= 4 && ((xs[2] + 65535) >> 16) <= X && X <= (xs[3] >> 16)) return true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const Edge &e = E[i];
        if (e.ymajor) {
            const int k = (y - e.ly) * e.sy;
            if (k >= 0 && k <= e.dmaj && x == e.lx + vkc::bres_minor(k, e.dmaj, e.dmin)) return true;
        } else {
            const int k = x - e.lx;
            if (k >= 0 && k <= e.dmaj && y == e.ly + e.sy * vkc::bres_minor(k, e.dmaj, e.dmin)) return true;
        }
    }
    return false;
}

// The host side of one call.  reserve() the vertex total, add() the contours, layout() + stage() the two tables among the
// caller's own in a vkx_tables, launch() after the block's copy, finish() last.  A contour of at most kCross vertices cannot
// cross a scanline more often than k_spans holds, so only calls with a larger one clear the overflow flag, read it back and
// synchronise for it; every other call returns with its kernels queued.
template <int kCross>
struct Raster {
    std::vector<PolyEdge> edges;
    std::vector<Item> items;
    long long steps = 0;           // outline steps of all edges
    bool may_overflow = false;
    size_t e_off = 0, i_off = 0;   // the tables in the caller's vkx_tables

    // false: too many vertices (an edge index would not fit an Item)
    bool reserve(long long total_pts)
    {
        if (total_pts < 0 || total_pts >= 0x3fffffff) return false;
        edges.reserve((size_t)total_pts);
        return true;
    }
    // One closed contour of npts >= 1 vertices (x, y), moved by (dx, dy): the edges carry `tag` (poly) and `target` (pad), the
    // items cover its scanlines inside [y_lo, y_hi).  false: the outlines are too long (a step index would not fit an int).
    bool add(const int32_t *pts, int npts, int tag, int target, int y_lo = INT_MIN, int y_hi = INT_MAX, int dx = 0, int dy = 0)
    {
        const size_t begin = edges.size();
        edges.resize(begin + (size_t)npts);
        int ymin = INT_MAX, ymax = INT_MIN;
        build_edges(pts, npts, dx, dy, tag, target, edges.data() + begin, &steps, &ymin, &ymax);
        if (steps >= 0x7fffffff) return false;
        may_overflow = may_overflow || npts > kCross;
        for (int y = std::max(ymin, y_lo); y < std::min(ymax, y_hi); y++)
            items.push_back(Item{(int)begin, (int)begin + npts, y, target, tag});
        return true;
    }

    void layout(vkx_tables &tab)
    {
        e_off = tab.add(sizeof(PolyEdge) * edges.size());
        i_off = tab.add(sizeof(Item) * items.size());
    }
    void stage(const vkx_tables &tab) const    // after tab.take()
    {
        if (!edges.empty()) memcpy(tab.at<PolyEdge>(e_off), edges.data(), sizeof(PolyEdge) * edges.size());
        if (!items.empty()) memcpy(tab.at<Item>(i_off), items.data(), sizeof(Item) * items.size());
    }
    // dev: where the vkx_tables block went.  idle_spans: the span kernel is launched even without an item (one idle workgroup),
    // for callers whose launches per call must not depend on their polygons.
    template <class Sink>
    int launch(vkx_ctx *ctx, const unsigned char *dev, int *overflow, const Sink &sink, const char *outline_name,
               const char *spans_name, bool idle_spans) const
    {
        const PolyEdge *d_edges = (const PolyEdge *)(dev + e_off);
        const Item *d_items = (const Item *)(dev + i_off);
        if (may_overflow) VKX_HIP(hipMemsetAsync(overflow, 0, sizeof(int), ctx->stream));      // (only such calls can set it, and only they read it)
        if (steps > 0) {
            { VKX_TIMED(ctx, outline_name); k_outline<Sink><<<vkx_blocks((size_t)steps, 256), 256, 0, ctx->stream>>>(d_edges, (int)edges.size(), (int)steps, sink); }
            VKX_LAUNCH_CHECK();
        }
        if (!items.empty() || idle_spans) {
            { VKX_TIMED(ctx, spans_name); k_spans<Sink, kCross><<<vkx_blocks(items.size(), 4), 256, 0, ctx->stream>>>(d_edges, d_items, (int)items.size(), sink, overflow); }
            VKX_LAUNCH_CHECK();
        }
        return VKX_OK;
    }
    // `what`: the subject of the message in the caller's words ("a polygon")
    int finish(vkx_ctx *ctx, const int *overflow, const char *what) const
    {
        if (!may_overflow) return VKX_OK;
        int flag = 0;
        VKX_HIP(hipMemcpyAsync(&flag, overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        VKX_HIP(hipStreamSynchronize(ctx->stream));
        if (flag) {
            vkx_set_error("%s has more than %d edge crossings on one scanline", what, kCross);
            return VKX_ERR_UNSUPPORTED;
        }
        return VKX_OK;
    }
};

constexpr int kPaintCross = 64; // crossings of one polygon on one scanline handled by the batched paths (a page's polygons are small)
constexpr int kPolyCross = 512; // ... by the single polygon of vkx_fill_poly_mask_u8 (32 KB of LDS a workgroup)

} // namespace vkp
