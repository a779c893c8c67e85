// The device half of cv.resize: ONE destination pixel of every interpolation, each stated once for every site that resizes --
// the direct kernels of resize.hip, the glyph planes of seal_fill.hip (k_seal_planes), the text lines of text_line.hip, the batched
// region resize of region_flatten.hip (k_region_resize) and the label shrink of crop.hip.  The batched record kernels, whose mode
// differs from record to record, reach their pixel through planned_pixel_u8 / planned_pixel_f32 at the end.  A site hands its source over as an accessor, which
// carries everything the site does to a sample on the way in: the pitch, the (m > 0) * 255 of a mask, the any-channel test of a
// 3-channel glyph.  The accessor is asked for clipped coordinates only.  The order of every float32 sum and the int32 wrap of the
// fixed-point sums are the oracle's (oracle/vkx_oracle.c); the library is built with -ffp-contract=off.  The host half (axis
// tables, routing rule, table blocks and their views) is vkx_resize_axes.h; k_resize_sep of resize.hip is the separable form of
// the tap pixels below.
#pragma once
#include "vkx_resize_axes.h"

namespace vkd {

__device__ __forceinline__ int clip_index(int x, int n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

// INTER_NEAREST: min(floor(d * scale), size - 1), scale in double.  INTER_NEAREST_EXACT (resizeNN_bitexact): 16.16 arithmetic.
__device__ __forceinline__ int nearest_index(int d, double scale, int ssize) { return min((int)floor(d * scale), ssize - 1); }
__device__ __forceinline__ int nearest_exact_index(int d, int step, int start, int ssize)
{
    return min((int)(((long long)step * d + start) >> 16), ssize - 1);
}

// INTER_CUBIC (KS = 4, taps from s - 1) and INTER_LANCZOS4 (KS = 8, taps from s - 3) on uint8: KS x KS taps a channel, 11-bit
// coefficients, int32 accumulation with wrap (like the int accumulators of the reference implementation), (sum + 2^21) >> 22,
// saturated.  load(y, b): byte b of source row y; x0, y0: the pixel's axis offsets; xa / yb: its own KS coefficients.
// The 24-bit multiply has the low 32 bits of the 32-bit product, at full rate, because both operands fit 24 bits signed: b is a
// short, and a row of coefficients is either an ordinary one (sum of |a| < 2^12, so |hsum| < 255 * 2^12 < 2^20) or the NaN column
// of LANCZOS4 (one tap saturated to -32768, the others 0: |hsum| <= 255 * 32768 < 2^23).
template <int CN, int KS, class Load>
__device__ __forceinline__ void taps_pixel_u8(Load load, int sh, int sw, int x0, int y0, const short *__restrict__ xa,
                                              const short *__restrict__ yb, uint8_t *out)
{
    constexpr int LEFT = KS / 2 - 1;
    int sx[KS], ax[KS];
#pragma unroll
    for (int j = 0; j < KS; j++) { sx[j] = clip_index(x0 - LEFT + j, sw) * CN; ax[j] = xa[j]; }
    unsigned acc[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) acc[c] = 0;
    const auto source_row = [&](int k) {
        const int row = clip_index(y0 - LEFT + k, sh);
        const int b = yb[k];
#pragma unroll
        for (int c = 0; c < CN; c++) {
            unsigned hsum = 0;
#pragma unroll
            for (int j = 0; j < KS; j++) hsum += (unsigned)(load(row, sx[j] + c) * ax[j]);
            acc[c] += (unsigned)__mul24((int)hsum, b);
        }
    };
    if constexpr (KS == 4) {                    // (the 4 rows unrolled, the 8 rows left to the compiler: as each was tuned)
#pragma unroll
        for (int k = 0; k < KS; k++) source_row(k);
    } else {
        for (int k = 0; k < KS; k++) source_row(k);
    }
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = (uint8_t)clamp_u8(((int)(acc[c] + (1u << 21))) >> 22);
}

// ... on float32: load(y, x); every sum left to right, rows first
template <int KS, class Load>
__device__ __forceinline__ float taps_pixel_f32(Load load, int sh, int sw, int x0, int y0, const float *__restrict__ xc,
                                                const float *__restrict__ yc)
{
    constexpr int LEFT = KS / 2 - 1;
    int sx[KS];
    float ax[KS];
#pragma unroll
    for (int j = 0; j < KS; j++) { sx[j] = clip_index(x0 - LEFT + j, sw); ax[j] = xc[j]; }
    float v = 0.f;
    const auto source_row = [&](int k) {
        const int row = clip_index(y0 - LEFT + k, sh);
        float hsum = load(row, sx[0]) * ax[0];
#pragma unroll
        for (int j = 1; j < KS; j++) { const float t = load(row, sx[j]) * ax[j]; hsum = hsum + t; }
        const float term = hsum * yc[k];
        v = k == 0 ? term : v + term;
    };
    if constexpr (KS == 4) {
#pragma unroll
        for (int k = 0; k < KS; k++) source_row(k);
    } else {
        for (int k = 0; k < KS; k++) source_row(k);
    }
    return v;
}

// INTER_LINEAR on uint8: 2 x 2 taps, horizontal pass in int32 with 11-bit coefficients, OpenCV's vertical rounding
// uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2).  load(y, b) as for the tap pixel.
template <int CN, class Load>
__device__ __forceinline__ void linear_pixel_u8(Load load, int sh, int sw, int x0, int y0, const short *__restrict__ xa,
                                                const short *__restrict__ yb, uint8_t *out)
{
    const int sx0 = x0 * CN, sx1 = clip_index(x0 + 1, sw) * CN;
    const int a0 = xa[0], a1 = xa[1], b0 = yb[0], b1 = yb[1];
    const int r0 = clip_index(y0, sh), r1 = clip_index(y0 + 1, sh);
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int h0 = load(r0, sx0 + c) * a0 + load(r0, sx1 + c) * a1;
        const int h1 = load(r1, sx0 + c) * a0 + load(r1, sx1 + c) * a1;
        out[c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
    }
}

// INTER_LINEAR on float32 (what INTER_LINEAR_EXACT falls back to for a ScoreMap): the weights computed per pixel; load(y, x)
template <class Load>
__device__ __forceinline__ float linear_pixel_f32(Load load, int sh, int sw, int dy, int dx, double scale_x, double scale_y)
{
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int y0 = (int)floorf(fy);
    fy -= y0;
    if (y0 < 0) { y0 = 0; fy = 0; }
    if (y0 >= sh - 1) { y0 = sh - 1; fy = 0; }
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int x0 = (int)floorf(fx);
    fx -= x0;
    if (x0 < 0) { x0 = 0; fx = 0; }
    if (x0 >= sw - 1) { x0 = sw - 1; fx = 0; }
    const int x1 = clip_index(x0 + 1, sw), y1 = clip_index(y0 + 1, sh);
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
    const float p0 = load(y0, x0) * a0, p1 = load(y0, x1) * a1, q0 = load(y1, x0) * a0, q1 = load(y1, x1) * a1;
    const float h0 = p0 + p1, h1 = q0 + q1;
    const float t0 = h0 * b0, t1 = h1 * b1;
    return t0 + t1;
}

// INTER_LINEAR_EXACT on uint8 (resize_bitExact): 8.8 weights, 16.16 vertical rounding; outside the ranges [p0, p1) of x and
// [p2, p3) of y both taps sit on the first / last source sample.  load(y, below, x, c): channel c of source pixel (y + below, x),
// below 0 or 1 -- a site that keeps a row pointer steps it by one pitch instead of multiplying again.
template <int CN, class Load>
__device__ __forceinline__ void linear_exact_pixel_u8(Load load, const LinearExactView &t, const int p[4], int dh, int dw, int dy, int dx,
                                                      uint8_t *out)
{
    const int xmin = p[0], xmax = p[1], ymin = p[2], ymax = p[3];
    const bool two = dy >= ymin && dy < ymax;
    const int r0 = dy < ymin ? 0 : (dy >= ymax ? t.yofs[dh - 1] : t.yofs[dy]);
    const int xa = dx < xmin ? 0 : (dx >= xmax ? t.xofs[dw - 1] : t.xofs[dx]);
    const bool xin = dx >= xmin && dx < xmax;
    const unsigned w1 = xin ? (unsigned)t.xw[dx] : 0u, w0 = 256u - w1;
    const int xb = xin ? xa + 1 : xa;
    const unsigned b1 = two ? (unsigned)t.yw[dy] : 0u, b0 = 256u - b1;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const unsigned h0 = w0 * load(r0, 0, xa, c) + w1 * load(r0, 0, xb, c);
        unsigned r;
        if (two) {
            const unsigned h1 = w0 * load(r0, 1, xa, c) + w1 * load(r0, 1, xb, c);
            r = (h0 * b0 + h1 * b1 + (1u << 15)) >> 16;
        } else {
            r = (h0 + 128u) >> 8;
        }
        out[c] = (uint8_t)(r > 255u ? 255u : r);
    }
}

// the exact 2 x 2 shrink of a uint8 plane, which cv.resize routes to INTER_AREA: (sum + 2) >> 2.  at(y, x, c): channel c of the
// pixel's 2 x 2 source box (box coordinates, as for area_fast_* below)
template <int CN, class At>
__device__ __forceinline__ void half_pixel_u8(At at, uint8_t *out)
{
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = (uint8_t)((at(0, 0, c) + at(0, 1, c) + at(1, 0, c) + at(1, 1, c) + 2) >> 2);
}

// INTER_AREA at integer factors (cv::ResizeAreaFast): one destination sample from its isx x isy source box, the box read
// through at(y, x) (box coordinates).  uint8: (sum + 2) >> 2 at 2 x 2, else cvRound(sum * (1.f / area)); float32:
// (a + b) + (c + d) then * 0.25f at 2 x 2, else the row-major box summed four samples at a time.  Every box sample is
// read exactly once.
template <class At>
__device__ __forceinline__ uint8_t area_fast_u8(At at, int isx, int isy)
{
    int sum = 0;
    for (int y = 0; y < isy; y++)
        for (int x = 0; x < isx; x++) sum += at(y, x);
    const int r = (isx == 2 && isy == 2) ? (sum + 2) >> 2 : cv_round((float)sum * (1.f / (isx * isy)));
    return (uint8_t)clamp_u8(r);
}
template <class At>
__device__ __forceinline__ float area_fast_f32(At at, int isx, int isy)
{
    if (isx == 2 && isy == 2) {          // the vector body of the 2 x 2 case pairs the rows
        const float top = at(0, 0) + at(0, 1);
        const float bottom = at(1, 0) + at(1, 1);
        const float s4 = top + bottom;
        return s4 * 0.25f;
    }
    const int area = isx * isy;
    float sum = 0;
    int k = 0;
    for (; k <= area - 4; k += 4) {      // the reference sums the row-major box four samples at a time
        const float a0 = at(k / isx, k % isx), a1 = at((k + 1) / isx, (k + 1) % isx);
        const float a2 = at((k + 2) / isx, (k + 2) % isx), a3 = at((k + 3) / isx, (k + 3) % isx);
        float g = a0 + a1;
        g = g + a2;
        g = g + a3;
        sum = sum + g;
    }
    for (; k < area; k++) sum = sum + at(k / isx, k % isx);
    return sum * (1.f / area);
}

// INTER_AREA, fractional scale (cv::ResizeArea): the weighted runs of the pixel's column and row (AreaView), float32 sums left
// to right, rows first; out[c] is the float32 sum (F32) or cvRound of it, saturated (uint8).  load(y, x, c) returns float.
template <int CN, bool F32, class Load, class Out>
__device__ __forceinline__ void area_pixel(Load load, const AreaView &t, int dy, int dx, Out *out)
{
    const int x0 = t.xstart[dx], x1 = t.xstart[dx + 1], y0 = t.ystart[dy], y1 = t.ystart[dy + 1];
    float sum[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) sum[c] = 0.f;
    for (int j = y0; j < y1; j++) {
        const float beta = t.yal[j];
        float buf[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) buf[c] = 0.f;
        for (int k = x0; k < x1; k++) {
            const float alpha = t.xal[k];
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const float w = load(t.ysi[j], t.xsi[k], c) * alpha;
                buf[c] = buf[c] + w;
            }
        }
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const float w = beta * buf[c];
            sum[c] = j == y0 ? w : sum[c] + w;
        }
    }
#pragma unroll
    for (int c = 0; c < CN; c++) {
        if constexpr (F32) out[c] = sum[c];
        else out[c] = (uint8_t)clamp_u8(cv_round(sum[c]));
    }
}

// ---- a PlannedResize (vkx_resize_axes.h) to its pixel: the function above its plan names, on the view of its table block.  `tabs`:
// the staged block the job's tab_off counts from.  The modes are the ones the codes of ResizePlanner::known_interpolation reach.
// One uint8 pixel of CN channels.  px(y, b): byte b = x * CN + c of source row y.
template <int CN, class Px>
__device__ void planned_pixel_u8(const PlannedResize &j, const unsigned char *tabs, int dy, int dx, Px px, uint8_t *out)
{
    const int sh = j.sh, sw = j.sw, dh = j.dh, dw = j.dw;
    const int *p = j.plan.p;
    const unsigned char *tab = tabs + j.tab_off;
    switch (j.plan.mode) {
    case M_COPY:
#pragma unroll
        for (int c = 0; c < CN; c++) out[c] = (uint8_t)px(dy, dx * CN + c);
        break;
    case M_NEAREST_EXACT: {
        const int sx = nearest_exact_index(dx, p[0], p[1], sw), sy = nearest_exact_index(dy, p[2], p[3], sh);
#pragma unroll
        for (int c = 0; c < CN; c++) out[c] = (uint8_t)px(sy, sx * CN + c);
        break;
    }
    case M_LINEAR_EXACT_U8:
        linear_exact_pixel_u8<CN>([&](int y, int below, int x, int c) { return (unsigned)px(y + below, x * CN + c); },
                                  LinearExactView::of(tab, dh, dw), p, dh, dw, dy, dx, out);
        break;
    case M_HALF_U8: half_pixel_u8<CN>([&](int y, int x, int c) { return px(2 * dy + y, (2 * dx + x) * CN + c); }, out); break;
    case M_TAPS:
        if (j.plan.ks == 4) {
            const TapView<short> t(tab, 4, dh, dw);
            taps_pixel_u8<CN, 4>(px, sh, sw, t.xofs[dx], t.yofs[dy], t.xcoef + 4 * dx, t.ycoef + 4 * dy, out);
        } else {
            const TapView<short> t(tab, 8, dh, dw);
            taps_pixel_u8<CN, 8>(px, sh, sw, t.xofs[dx], t.yofs[dy], t.xcoef + 8 * dx, t.ycoef + 8 * dy, out);
        }
        break;
    case M_AREA_FAST:
#pragma unroll
        for (int c = 0; c < CN; c++)
            out[c] = area_fast_u8([&](int y, int x) { return px(dy * p[1] + y, (dx * p[0] + x) * CN + c); }, p[0], p[1]);
        break;
    default:                                    // M_AREA
        area_pixel<CN, false>([&](int y, int x, int c) { return (float)px(y, x * CN + c); }, AreaView(tab, dh, dw), dy, dx, out);
        break;
    }
}

// ... and one float32 pixel, as ScoreMap.to_resized_score_map leaves it: clipped to [0, 1] unless nothing was resized.  px(y, x).
template <class Px>
__device__ float planned_pixel_f32(const PlannedResize &j, const unsigned char *tabs, int dy, int dx, Px px)
{
    const int sh = j.sh, sw = j.sw, dh = j.dh, dw = j.dw;
    const int *p = j.plan.p;
    const unsigned char *tab = tabs + j.tab_off;
    float v = 0.f;
    switch (j.plan.mode) {
    case M_COPY: return px(dy, dx);
    case M_NEAREST_EXACT:
        v = px(nearest_exact_index(dy, p[2], p[3], sh), nearest_exact_index(dx, p[0], p[1], sw));
        break;
    case M_LINEAR_F32: v = linear_pixel_f32(px, sh, sw, dy, dx, j.plan.scale_x, j.plan.scale_y); break;
    case M_TAPS:
        if (j.plan.ks == 4) {
            const TapView<float> t(tab, 4, dh, dw);
            v = taps_pixel_f32<4>(px, sh, sw, t.xofs[dx], t.yofs[dy], t.xcoef + 4 * dx, t.ycoef + 4 * dy);
        } else {
            const TapView<float> t(tab, 8, dh, dw);
            v = taps_pixel_f32<8>(px, sh, sw, t.xofs[dx], t.yofs[dy], t.xcoef + 8 * dx, t.ycoef + 8 * dy);
        }
        break;
    case M_AREA_FAST: v = area_fast_f32([&](int y, int x) { return px(dy * p[1] + y, dx * p[0] + x); }, p[0], p[1]); break;
    default:                                    // M_AREA
        area_pixel<1, true>([&](int y, int x, int) { return px(y, x); }, AreaView(tab, dh, dw), dy, dx, &v);
        break;
    }
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);      // np.clip(mat, 0, 1); a NaN stays
}

} // namespace vkd
