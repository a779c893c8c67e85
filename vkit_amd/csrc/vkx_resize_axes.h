// The host half of cv.resize, stated once for every site that resizes (resize.hip, the batched glyph resize of seal_fill.hip, the
// batched region resize of region_flatten.hip): the axis tables (bit for bit oracle/vkx_oracle.c's), the rule that routes a
// request to a kernel (plan_resize), and the blocks the tables travel to the device in -- a packer that writes a block and the
// view a kernel, or the host that launches it, reads the block through.  The batched record kernels (seal_fill.hip, text_line.hip)
// carry a resize as a PlannedResize and plan, lay out and pack all of a call's with one ResizePlanner.  The device half is
// vkx_resize_pixel.h.
#pragma once
#include "vkx_internal.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace vkd {

// cvRound of a host float: ties to even, "integer indefinite" (INT_MIN) for NaN and out-of-range values -- a LANCZOS4
// coefficient can be NaN (fraction rounding up to exactly 1.0f makes one tap 0 / 0), and saturate_cast<short> of that
// is -32768 in cv2, not whatever a plain (int) cast of NaN yields.
inline int cv_round_host(float v)
{
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)std::nearbyint((double)v);
}
inline short fixed_coef(float c)              // 11-bit fixed point, saturate_cast<short>
{
    const int r = cv_round_host(c * 2048.f);
    return (short)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
}

inline void cubic_coeffs(float x, float c[4])
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// interpolateLanczos4 (imgproc): 8 taps s-3 .. s+4
inline void lanczos4_coeffs(float x, float c[8])
{
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const double pi = 3.1415926535897932384626433832795;
    if (x < FLT_EPSILON) {
        for (int i = 0; i < 8; i++) c[i] = 0;
        c[3] = 1;
        return;
    }
    float sum = 0;
    const double y0 = -(x + 3) * pi * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
    for (int i = 0; i < 8; i++) {
        const double y = -(x + 3 - i) * pi * 0.25;
        c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        sum += c[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) c[i] *= sum;
}

// One axis of a tap interpolation: ks = 2 INTER_LINEAR (taps s, s + 1; `horizontal` pins the first and last columns as
// HResizeLinear's tables do), 4 INTER_CUBIC (taps from s - 1), 8 INTER_LANCZOS4 (taps from s - 3).
struct AxisTable {
    std::vector<int> ofs;      // floor of the source coordinate
    std::vector<float> coef;   // [n][ks]
    std::vector<short> icoef;  // [n][ks], cvRound(coef * 2048)
};

inline void build_axis(int ks, int ssize, int dsize, AxisTable *t, bool horizontal = false)
{
    t->ofs.resize(dsize); t->coef.resize((size_t)dsize * ks); t->icoef.resize((size_t)dsize * ks);
    const double inv_scale = (double)dsize / ssize;
    const double scale = 1. / inv_scale;
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s0 = (int)std::floor(f);
        f -= s0;
        float *c = &t->coef[(size_t)d * ks];
        if (ks == 2) {
            if (horizontal && s0 < 0) { f = 0; s0 = 0; }
            if (horizontal && s0 >= ssize - 1) { f = 0; s0 = ssize - 1; }
            c[0] = 1.f - f; c[1] = f;
        } else if (ks == 4) {
            cubic_coeffs(f, c);
        } else {
            lanczos4_coeffs(f, c);
        }
        t->ofs[d] = s0;
        for (int k = 0; k < ks; k++) t->icoef[(size_t)d * ks + k] = fixed_coef(c[k]);
    }
}

// INTER_LINEAR_EXACT on uint8 (resize_bitExact): per axis (offset, 8.8 weight of the second sample) and the range
// [mn, mx) of destination indices that interpolate; outside it the first / last source sample is copied
inline void build_linear_exact_axis(int ssize, int dsize, int *ofs, int *w1, int *dmin, int *dmax)
{
    const double inv_scale = (double)dsize / ssize, scale = 1.0 / inv_scale;
    int mn = 0, mx = dsize;
    for (int d = 0; d < dsize; d++) {
        const double fval = scale * ((double)d + 0.5) - 0.5;
        int ival = (int)std::floor(fval);
        w1[d] = 0;
        if (ival >= 0 && ssize > 1) {
            if (ival < ssize - 1) w1[d] = (int)std::nearbyint((fval - (double)ival) * 256.0);
            else { ival = ssize - 1; mx = std::min(mx, d); }
        } else { mn = std::max(mn, d + 1); ival = 0; }
        ofs[d] = ival;
    }
    if (mx < mn) mx = mn;
    *dmin = mn; *dmax = mx;
}

// INTER_AREA, fractional scale (ResizeArea): computeResizeAreaTab's (source index, weight) runs per destination index
struct AreaTab {
    std::vector<int> start;    // [dsize + 1] first entry of every destination index
    std::vector<int> si;
    std::vector<float> alpha;
};

inline void build_area_tab(int ssize, int dsize, double scale, AreaTab *t)
{
    t->start.assign(dsize + 1, 0); t->si.clear(); t->alpha.clear();
    for (int dx = 0; dx < dsize; dx++) {
        t->start[dx] = (int)t->si.size();
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) { t->si.push_back(sx1 - 1); t->alpha.push_back((float)((sx1 - fsx1) / cell)); }
        for (int sx = sx1; sx < sx2; sx++) { t->si.push_back(sx); t->alpha.push_back((float)(1.0 / cell)); }
        if (fsx2 - sx2 > 1e-3) { t->si.push_back(sx2); t->alpha.push_back((float)(std::min(std::min(fsx2 - sx2, 1.), cell) / cell)); }
    }
    t->start[dsize] = (int)t->si.size();
}

// ---- the routing rule: which kernel cv.resize(src (sh, sw) -> (dh, dw), interpolation) is, on float32 or uint8 ----------------
enum ResizeMode {
    M_COPY,                    // (no resize at all: the batched sites' equal shapes; plan_resize never returns it)
    M_NEAREST, M_NEAREST_EXACT, M_LINEAR_U8, M_LINEAR_F32, M_LINEAR_EXACT_U8, M_HALF_U8, M_TAPS, M_AREA_FAST, M_AREA,
    M_REFUSED_AREA_ENLARGES,   // INTER_AREA is implemented for shrinking only (the reference samples it only then)
    M_REFUSED_UNKNOWN          // not an interpolation code of cv2
};

struct ResizePlan {
    int mode = M_COPY;
    int ks = 0;                          // M_TAPS: 4 or 8
    int p[4] = {0, 0, 0, 0};             // M_NEAREST_EXACT: the 16.16 step and start of x, then of y; M_AREA_FAST: the factors
                                         // of x and y; M_LINEAR_EXACT_U8: [xmin, xmax), [ymin, ymax) -- set when the block is packed
    double scale_x = 1.0, scale_y = 1.0; // source pixels per destination pixel
    bool refused() const { return mode >= M_REFUSED_AREA_ENLARGES; }
};

inline ResizePlan plan_resize(bool f32, int interpolation, int sh, int sw, int dh, int dw)
{
    ResizePlan r;
    r.scale_x = 1. / ((double)dw / sw); r.scale_y = 1. / ((double)dh / sh);
    const bool half = sw == 2 * dw && sh == 2 * dh;
    switch (interpolation) {
    case VKX_INTER_NEAREST: r.mode = M_NEAREST; return r;
    case VKX_INTER_NEAREST_EXACT:
        r.mode = M_NEAREST_EXACT;
        r.p[0] = (int)((((long long)sw << 16) + dw / 2) / dw); r.p[1] = r.p[0] / 2 - sw % 2;
        r.p[2] = (int)((((long long)sh << 16) + dh / 2) / dh); r.p[3] = r.p[2] / 2 - sh % 2;
        return r;
    case VKX_INTER_CUBIC: r.mode = M_TAPS; r.ks = 4; return r;
    case VKX_INTER_LANCZOS4: r.mode = M_TAPS; r.ks = 8; return r;
    case VKX_INTER_LINEAR:
    case VKX_INTER_LINEAR_EXACT:         // no bit-exact float32 path in cv.resize: INTER_LINEAR_EXACT falls back to INTER_LINEAR
        if (!half) {
            r.mode = f32 ? M_LINEAR_F32 : (interpolation == VKX_INTER_LINEAR ? M_LINEAR_U8 : M_LINEAR_EXACT_U8);
            return r;
        }
        if (!f32) { r.mode = M_HALF_U8; return r; }
        /* fallthrough: cv.resize routes the exact 2 x 2 shrink of a float32 plane to INTER_AREA */
    case VKX_INTER_AREA: {
        if (dw > sw || dh > sh) { r.mode = M_REFUSED_AREA_ENLARGES; return r; }
        const int isx = (int)std::nearbyint(r.scale_x), isy = (int)std::nearbyint(r.scale_y);
        if (std::fabs(r.scale_x - isx) < DBL_EPSILON && std::fabs(r.scale_y - isy) < DBL_EPSILON) {
            r.mode = M_AREA_FAST; r.p[0] = isx; r.p[1] = isy;
        } else {
            r.mode = M_AREA;
        }
        return r;
    }
    default: r.mode = M_REFUSED_UNKNOWN; return r;
    }
}

// ---- the table blocks.  A packer returns the bytes of its block and, given an address, writes the block there; the view of the
// same name is how the block is read.  No other code knows a block's layout.
template <class T> inline unsigned char *put_array(unsigned char *out, const T *v, size_t n)
{
    memcpy(out, v, sizeof(T) * n);
    return out + sizeof(T) * n;
}

// Tap block: int xofs[dw], yofs[dh]; CT xcoef[ks * dw], ycoef[ks * dh], CT = short (uint8 planes) or float.
template <class CT>
struct TapView {
    const int *xofs, *yofs;
    const CT *xcoef, *ycoef;
    __host__ __device__ TapView(const void *block, int ks, int dh, int dw)
        : xofs((const int *)block), yofs(xofs + dw), xcoef((const CT *)(yofs + dh)), ycoef(xcoef + (ptrdiff_t)ks * dw) {}
};
// `yofs_host`: a copy of the row offsets for the caller (resize.hip plans its separable tiles on them)
inline size_t pack_taps(int ks, bool f32, int sh, int sw, int dh, int dw, unsigned char *out, std::vector<int> *yofs_host = nullptr)
{
    const size_t bytes = (sizeof(int) + ks * (f32 ? sizeof(float) : sizeof(short))) * ((size_t)dw + dh);
    if (!out) return bytes;
    AxisTable tx, ty;
    build_axis(ks, sw, dw, &tx, true);
    build_axis(ks, sh, dh, &ty, false);
    out = put_array(put_array(out, tx.ofs.data(), dw), ty.ofs.data(), dh);
    if (f32) put_array(put_array(out, tx.coef.data(), tx.coef.size()), ty.coef.data(), ty.coef.size());
    else put_array(put_array(out, tx.icoef.data(), tx.icoef.size()), ty.icoef.data(), ty.icoef.size());
    if (yofs_host) yofs_host->swap(ty.ofs);
    return bytes;
}

// LINEAR_EXACT block: int xofs[dw], xw[dw], yofs[dh], yw[dh]; the four range ends go to range[4] (ResizePlan::p)
struct LinearExactView {
    const int *xofs, *xw, *yofs, *yw;
    __host__ __device__ static LinearExactView of(const void *block, int dh, int dw)
    {
        const int *xofs = (const int *)block;
        return LinearExactView{xofs, xofs + dw, xofs + 2 * (ptrdiff_t)dw, xofs + 2 * (ptrdiff_t)dw + dh};
    }
};
inline size_t pack_linear_exact(int sh, int sw, int dh, int dw, unsigned char *out, int range[4])
{
    const size_t bytes = 2 * sizeof(int) * ((size_t)dw + dh);
    if (!out) return bytes;
    int *x = (int *)out, *y = x + 2 * (size_t)dw;
    build_linear_exact_axis(sw, dw, x, x + dw, &range[0], &range[1]);
    build_linear_exact_axis(sh, dh, y, y + dh, &range[2], &range[3]);
    return bytes;
}

// AREA block: int xstart[dw + 1], ystart[dh + 1], xsi[nx], ysi[ny]; float xal[nx], yal[ny] with nx = xstart[dw], ny = ystart[dh]
struct AreaView {
    const int *xstart, *ystart, *xsi, *ysi;
    const float *xal, *yal;
    __host__ __device__ AreaView(const void *block, int dh, int dw, int nx, int ny)
        : xstart((const int *)block), ystart(xstart + dw + 1), xsi(ystart + dh + 1), ysi(xsi + nx), xal((const float *)(ysi + ny)),
          yal(xal + nx) {}
    // (on the device, where the block can be read: the entry counts are the last entries of the two start tables)
    __device__ AreaView(const void *block, int dh, int dw) : AreaView(block, dh, dw, ((const int *)block)[dw], ((const int *)block)[dw + 1 + dh]) {}
};
struct AreaTabs {
    AreaTab x, y;
    AreaTabs(int sh, int sw, int dh, int dw, double scale_x, double scale_y) { build_area_tab(sw, dw, scale_x, &x); build_area_tab(sh, dh, scale_y, &y); }
    size_t pack(unsigned char *out) const
    {
        const size_t bytes = sizeof(int) * (x.start.size() + y.start.size()) + (sizeof(int) + sizeof(float)) * (x.si.size() + y.si.size());
        if (!out) return bytes;
        out = put_array(put_array(out, x.start.data(), x.start.size()), y.start.data(), y.start.size());
        out = put_array(put_array(out, x.si.data(), x.si.size()), y.si.data(), y.si.size());
        put_array(put_array(out, x.alpha.data(), x.alpha.size()), y.alpha.data(), y.alpha.size());
        return bytes;
    }
};

// ---- one cv.resize of a batched call as its record carries it: the plan, where its table block lies and the two shapes.  The
// device reads it through planned_pixel_u8 / planned_pixel_f32 of vkx_resize_pixel.h.
struct PlannedResize {
    ResizePlan plan;                     // (M_COPY: equal shapes, nothing is resized)
    long long tab_off;                   // its table block, bytes from the start of the staged block (no block: 0)
    int sh, sw, dh, dw;
};

// All the resizes of one batched call.  plan() every job while the records are checked; layout() once, where the table blocks
// belong in the staged block; pack() once the block is taken.  The planner keeps the ADDRESS of every job, so the records stay
// where they are between plan() and pack() -- and they are copied to the staged block only AFTER pack(): packing a LINEAR_EXACT
// block is what writes the range ends into plan.p.
class ResizePlanner {
    struct Item {
        PlannedResize *job;
        bool f32;
        size_t bytes;                    // of its block, set by layout()
        std::unique_ptr<AreaTabs> area;  // M_AREA only
    };
    std::vector<Item> items;
    const char *entry;                   // the entry point a refusal is reported for

    // the bytes of a job's table block (none: 0); given an address, the block is written there
    static size_t pack_block(const Item &it, unsigned char *out)
    {
        PlannedResize &j = *it.job;
        switch (j.plan.mode) {
        case M_TAPS: return pack_taps(j.plan.ks, it.f32, j.sh, j.sw, j.dh, j.dw, out);
        case M_LINEAR_EXACT_U8: return pack_linear_exact(j.sh, j.sw, j.dh, j.dw, out, j.plan.p);
        case M_AREA: return it.area->pack(out);
        default: return 0;
        }
    }

public:
    explicit ResizePlanner(const char *entry_point) : entry(entry_point) {}

    // the interpolation codes the batched sites take
    static bool known_interpolation(int c)
    {
        return c == VKX_INTER_CUBIC || c == VKX_INTER_AREA || c == VKX_INTER_LANCZOS4 || c == VKX_INTER_LINEAR_EXACT || c == VKX_INTER_NEAREST_EXACT;
    }

    // cv.resize((sh, sw) -> (dh, dw)) on float32 or uint8 into `j`.  Equal shapes leave M_COPY and plan nothing.
    int plan(PlannedResize &j, bool f32, int interpolation, int sh, int sw, int dh, int dw)
    {
        j = PlannedResize{ResizePlan(), 0, sh, sw, dh, dw};
        if (sh == dh && sw == dw) return VKX_OK;
        j.plan = plan_resize(f32, interpolation, sh, sw, dh, dw);
        if (j.plan.refused()) {
            vkx_set_error(VKX_REQUIRE_FORMAT, entry, "INTER_AREA is for shrinking only");
            return VKX_ERR_INVALID;
        }
        items.push_back(Item{&j, f32, 0, nullptr});
        if (j.plan.mode == M_AREA) items.back().area.reset(new AreaTabs(sh, sw, dh, dw, j.plan.scale_x, j.plan.scale_y));
        return VKX_OK;
    }
    // add(bytes) -> the offset of a block of that size in the staged block (vkx_tables::add), asked once per job that has tables
    template <class Add>
    void layout(Add add)
    {
        for (Item &it : items)
            if ((it.bytes = pack_block(it, nullptr))) it.job->tab_off = (long long)add(it.bytes);
    }
    // ... and the blocks written at their offsets from `base`, the taken block
    void pack(unsigned char *base) const
    {
        for (const Item &it : items)
            if (it.bytes) pack_block(it, base + it.job->tab_off);
    }
};

} // namespace vkd
