// cv.resize INTER_CUBIC on uint8 (11-bit fixed point), the parts shared by resize.hip and the batched region resize of
// region_flatten.hip: the host-side axis tables and the device arithmetic of one destination pixel, each stated once.
#pragma once
#include "vkx_internal.h"

#include <climits>
#include <cmath>
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

struct AxisTable {
    std::vector<int> ofs;      // floor of the source coordinate
    std::vector<float> coef;   // [n][4]
    std::vector<short> icoef;  // [n][4], cvRound(coef * 2048)
};

inline void cubic_coeffs(float x, float c[4])
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

inline void build_axis(int ssize, int dsize, AxisTable *t)
{
    t->ofs.resize(dsize); t->coef.resize((size_t)dsize * 4); t->icoef.resize((size_t)dsize * 4);
    const double inv_scale = (double)dsize / ssize;
    const double scale = 1. / inv_scale;
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        const int s0 = (int)std::floor(f);
        f -= s0;
        t->ofs[d] = s0;
        cubic_coeffs(f, &t->coef[(size_t)d * 4]);
        for (int k = 0; k < 4; k++) {
            const int r = cv_round_host(t->coef[(size_t)d * 4 + k] * 2048.f);
            t->icoef[(size_t)d * 4 + k] = (short)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
        }
    }
}

__device__ __forceinline__ int clip_index(int x, int n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

// One destination pixel of the gather form: 4 x 4 taps a channel, int32 accumulation with wrap, (sum + 2^21) >> 22, saturated.
// load(y, b): byte b of source row y (both already clipped to the source); xa / yb: the pixel's own four coefficients.
template <int CN, class Load>
__device__ __forceinline__ void cubic_pixel_u8(Load load, int sh, int sw, int x0, int y0, const short *__restrict__ xa,
                                               const short *__restrict__ yb, uint8_t *out)
{
    int sx[4], ax[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { sx[j] = clip_index(x0 - 1 + j, sw) * CN; ax[j] = xa[j]; }
    unsigned acc[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) acc[c] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int row = clip_index(y0 - 1 + k, sh);
        const int b = yb[k];
#pragma unroll
        for (int c = 0; c < CN; c++) {
            unsigned hsum = 0; // int32 with wrap, like the int accumulators of the reference implementation
#pragma unroll
            for (int j = 0; j < 4; j++) hsum += (unsigned)(load(row, sx[j] + c) * ax[j]);
            acc[c] += (unsigned)__mul24((int)hsum, b);      // |hsum| < 2^20: same low 32 bits as the 32-bit product
        }
    }
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int r = ((int)(acc[c] + (1u << 21))) >> 22;
        out[c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
}

} // namespace vkd
