// The edge table of cv::fillPoly (CollectPolyEdges + the LINE_8 outline) and the device steps that walk it, shared by the
// polygon rasters of polygon.hip and the text-region masks of region_masks.hip: one definition, one raster.
#pragma once
#include "vkx_internal.h"
#include "vkx_cell.h"

#include <algorithm>

struct PolyEdge {
    int xa, ya, xb, yb;        // contour order
    int lx, ly, dmaj, dmin;    // Bresenham from the left end
    int sy, ymajor;
    int step_base;             // prefix of (dmaj + 1) over the edges
    int y0, y1;                // scanline range of the edge (y0 == y1: horizontal, not in the edge table)
    int poly, pad;             // batched paint: 1-based paint order of the polygon this edge belongs to
    long long x0_fix, dx_fix;  // 16.16 x at y0, dx per scanline
};

// Edge table of one closed contour (cv::fillPoly -> CollectPolyEdges + the LINE_8 outline).
static inline void build_edges(const int32_t *pts, int npts, int poly, PolyEdge *edges, long long *steps, int *ymin, int *ymax)
{
    for (int i = 0; i < npts; i++) {
        const int a = (i + npts - 1) % npts;
        PolyEdge &e = edges[i];
        e.xa = pts[2 * a]; e.ya = pts[2 * a + 1];
        e.xb = pts[2 * i]; e.yb = pts[2 * i + 1];
        int lx = e.xa, ly = e.ya, rx = e.xb, ry = e.yb;
        if (rx < lx) { std::swap(lx, rx); std::swap(ly, ry); }
        const int dx = rx - lx, dy = ry - ly, ady = dy < 0 ? -dy : dy;
        e.lx = lx; e.ly = ly; e.sy = dy < 0 ? -1 : 1;
        e.ymajor = ady > dx;
        e.dmaj = e.ymajor ? ady : dx;
        e.dmin = e.ymajor ? dx : ady;
        e.step_base = (int)*steps;
        *steps += e.dmaj + 1;
        e.y0 = std::min(e.ya, e.yb); e.y1 = std::max(e.ya, e.yb);
        e.poly = poly; e.pad = 0;
        if (e.ya != e.yb) {
            const long long xa = (long long)e.xa << 16, xb = (long long)e.xb << 16;
            e.dx_fix = (xb - xa) / (long long)(e.yb - e.ya);
            e.x0_fix = e.ya < e.yb ? xa : xb;
            *ymin = std::min(*ymin, e.y0); *ymax = std::max(*ymax, e.y1);
        } else {
            e.dx_fix = 0; e.x0_fix = 0;
        }
    }
}

constexpr int kPaintCross = 64; // crossings of one polygon on one scanline handled by the batched (one wave a scanline) paths

namespace vkp {

// the edge that outline step t belongs to (step_base is a prefix sum), and the pixel of that step
__device__ __forceinline__ PolyEdge edge_of_step(const PolyEdge *__restrict__ edges, int nedges, int t)
{
    int lo = 0, hi = nedges - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (edges[mid].step_base <= t) lo = mid; else hi = mid - 1;
    }
    return edges[lo];
}

__device__ __forceinline__ void edge_pixel(const PolyEdge &e, int t, int &x, int &y)
{
    const int k = t - e.step_base;
    const int m = vkc::bres_minor(k, e.dmaj, e.dmin);
    x = e.ymajor ? e.lx + m : e.lx + k;
    y = e.ymajor ? e.ly + e.sy * k : e.ly + e.sy * m;
}

// One wave, one (polygon, scanline), in two steps that the workgroup's waves take together (each ends in __syncthreads).  xs /
// sorted: kPaintCross words of LDS each and `count` one word, all the wave's own; `count` is zeroed by the caller before a barrier.
// wave_crossings: lanes test the polygon's edges [edge_begin, edge_end) and collect the 16.16 crossings of the half-open edges
// (y0 <= y < y1) in xs; returns their number, which may exceed the kPaintCross that were kept (the caller's overflow).
__device__ __forceinline__ int wave_crossings(const PolyEdge *__restrict__ edges, int edge_begin, int edge_end, int y, long long *xs,
                                              int *count, int lane)
{
    for (int i = edge_begin + lane; i < edge_end; i += 64) {
        const PolyEdge &e = edges[i];
        if (e.y0 != e.y1 && e.y0 <= y && y < e.y1) {
            const int slot = atomicAdd(count, 1);
            if (slot < kPaintCross) xs[slot] = e.x0_fix + (long long)(y - e.y0) * e.dx_fix;
        }
    }
    __syncthreads();
    return *count;
}

// wave_rank: the n <= kPaintCross crossings ranked by counting into `sorted` (no sort loop: rank = number of crossings that
// precede it; the tie-break on the slot keeps the ranking a permutation)
__device__ __forceinline__ void wave_rank(const long long *xs, long long *sorted, int n, int lane)
{
    if (lane < n) {
        const long long v = xs[lane];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const long long u = xs[j];
            rank += (u < v) || (u == v && j < lane);
        }
        sorted[rank] = v;
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

} // namespace vkp
