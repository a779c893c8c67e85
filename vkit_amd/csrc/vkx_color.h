// cv.cvtColor RGB <-> HSV_FULL on uint8 (element/image.py:188-202,771-814; photometric/color.py:93-116), shared by the
// single-stage kernels (photo.hip) and the fused chain kernel (fused.hip).  Must agree bit for bit with
// oracle/vkx_oracle.c: integer LUT division forwards, the scalar float32 HSV2RGB_native formula (no FMA) backwards.
//
// The header also compiles for the host without HIP (tools/hue_forms_check.cpp): the arithmetic below is plain C++ and the
// device builtins sit behind the helpers of vkd::hc, each with a plain C++ fallback, so the exhaustive checker runs the
// very source lines the kernels compile.  Build it with -ffp-contract=off, like the library.
#ifndef VKX_COLOR_H_
#define VKX_COLOR_H_

#ifdef __HIPCC__
#include "vkx_internal.h"
#define VKX_COLOR_FN __device__ __forceinline__
#define VKX_COLOR_TABLE __device__ constexpr
#else
#include <stdint.h>
#define VKX_COLOR_FN static inline
#define VKX_COLOR_TABLE static constexpr
#endif

namespace vkd {

// The builtins the colour arithmetic uses, and what each of them computes.
namespace hc {
VKX_COLOR_FN uint32_t f2u(float v) { return __builtin_bit_cast(uint32_t, v); }
VKX_COLOR_FN float u2f(uint32_t v) { return __builtin_bit_cast(float, v); }
VKX_COLOR_FN float abs(float v) { return __builtin_fabsf(v); }
VKX_COLOR_FN int max3(int a, int b, int c) { const int m = a > b ? a : b; return m > c ? m : c; }
VKX_COLOR_FN int min3(int a, int b, int c) { const int m = a < b ? a : b; return m < c ? m : c; }
// the low 24 bits of both factors, signed / unsigned; low 32 bits of the product
VKX_COLOR_FN int mul24(int a, int b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(a, b);
#else
    return (int)((uint32_t)((int)((uint32_t)a << 8) >> 8) * (uint32_t)((int)((uint32_t)b << 8) >> 8));
#endif
}
VKX_COLOR_FN uint32_t umul24(uint32_t a, uint32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umul24(a, b);
#else
    return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}
// round to nearest, ties to even (callers stay inside int32)
VKX_COLOR_FN int rint_even(float v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float2int_rn(v);
#else
    return (int)__builtin_rintf(v);      // the default rounding mode
#endif
}
// A table index through a vector register the optimiser does not look into (an empty asm statement on a VGPR).  The LDS
// tables of the kernels start at an address the compiler learns too late to fold: with the index's shift merged into other
// uses of the same value (4 * diff, (h6 >> 6) & ~3) the entry's address costs a shift, or a shift and a mask, AND an add of
// zero; kept apart it is one v_lshl_add_u32.
VKX_COLOR_FN int table_index(int v)
{
#ifdef __HIP_DEVICE_COMPILE__
    asm("" : "+v"(v));
#endif
    return v;
}
// v_perm_b32: result byte i is byte sel[i] of (hi : lo), 0 .. 3 from lo and 4 .. 7 from hi; 8 .. 11 replicate a sign bit,
// 12 gives 0x00, 13 and above 0xff
VKX_COLOR_FN uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 0xffu;
        uint32_t byte;
        if (s < 8) byte = (uint32_t)(both >> (8 * s)) & 0xffu;
        else if (s < 12) byte = ((both >> (16 * (s - 8) + 15)) & 1u) ? 0xffu : 0u;
        else byte = s == 12 ? 0u : 0xffu;
        out |= byte << (8 * i);
    }
    return out;
#endif
}
} // namespace hc

// sdiv[i] = cvRound((255 << 12) / i), hdiv[i] = cvRound((256 << 12) / (6 i)): both < 2^24, and diff, |hh| < 2^11, so the
// 24-bit multiplies (full rate) are exact.
// WRAP_H: leave the hue as computed, valid modulo 256 (callers that add a shift and reduce modulo 256 anyway).
// Otherwise the negative half is moved up by 256; the quotient then lies in 0..255 by construction (|hh| <= 5 diff before
// the division, so at most 213 after it, at least -43): saturate_cast has nothing to clamp.
// hround: what the hue product is rounded with, (1 << 11) + (k << 12) to get H + k out of the shift itself (a multiple of
// 4096 added before an arithmetic shift by 12 comes out as that many units after it; |product| < 2^21).
template <bool WRAP_H = false>
VKX_COLOR_FN void rgb2hsv_full(const int *sdiv, const int *hdiv, int r, int g, int b, int &H, int &S, int &V,
                               int hround = 1 << 11)
{
    const int v = hc::max3(b, g, r), vmin = hc::min3(b, g, r);
    const int diff = v - vmin;
    S = (hc::mul24(diff, sdiv[v]) + (1 << 11)) >> 12;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    int hh = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    // |hh| < 2^11 and hdiv < 2^24: the signed 24-bit multiply-add is exact (the intrinsic, not an asm statement with a
    // scalar operand: see mad_u24_ks in fused.hip)
    hh = hc::mul24(hh, hdiv[hc::table_index(diff)]) + hround;
    hh >>= 12;
    if (!WRAP_H) hh += hh < 0 ? 256 : 0;
    H = hh;
    V = v;
}

// Branch free: with s == 0 every candidate below is fv * 1.0f == fv, which is the reference's grey shortcut; H < 256
// keeps the sector in 0..5.  sector table (b, g, r): 0 (t1,t3,t0) 1 (t1,t0,t2) 2 (t3,t0,t1) 3 (t0,t2,t1) 4 (t0,t1,t3)
// 5 (t2,t1,t0) = (t1, odd ? t0 : t3, odd ? t2 : t0) rotated left by sector / 2.
// This is the restatement of the reference's formula, operation by operation; hsv2rgb_packed below is proven against it.
VKX_COLOR_FN void hsv2rgb_full(int H, int S, int V, int &r, int &g, int &b)
{
    const float s = S * (1.0f / 255.0f);
    const float fv = V * (1.0f / 255.0f);
    // h = H * 6 / 256 is exact in float32 (6 / 256 = 3 / 128, H * 6 < 2^11): its floor and fraction in integers
    const int h6 = hc::mul24(H, 6);
    const int sector = h6 >> 8;
    const float h = (float)(h6 & 255) * (1.0f / 256);
    const bool odd = sector & 1;
    const int rot = sector >> 1;
    // t2 = fv (1 - s h) serves the odd sectors, t3 = fv (1 - s (1 - h)) the even ones: only the one in use is evaluated
    const float t0 = fv;
    const float t1 = fv * (1.f - s);
    const float tt = fv * (1.f - s * (odd ? h : 1.f - h));
    const float u0 = t1, u1 = odd ? t0 : tt, u2 = odd ? tt : t0;
    const float fb = rot == 0 ? u0 : (rot == 1 ? u1 : u2);
    const float fg = rot == 0 ? u1 : (rot == 1 ? u2 : u0);
    const float fr = rot == 0 ? u2 : (rot == 1 ? u0 : u1);
    // 0 <= f <= 1, so round-half-even needs neither the cvRound range check nor the saturate_cast clamp
    r = hc::rint_even(fr * 255.0f);
    g = hc::rint_even(fg * 255.0f);
    b = hc::rint_even(fb * 255.0f);
}

// HSV_FULL -> RGB of the fused chain kernel: the results of hsv2rgb_full for every (H, S, V) in 0..255 (proven on all 2^24
// of them by tools/hue_forms_check.cpp, tests/test_hue_forms_exhaustive.py), arranged for the instruction mix of gfx950
// (float32 add / mul / fma and 32-bit add / sub / logic / shift right issue in about 2.5 cycles per wavefront; converts,
// compares, selects, shifts left, 24-bit multiplies and permutes in about 4.5):
//   * t0 * 255 rounds to V itself (V / 255 is within one ulp of the quotient, times 255 within one ulp of V): not evaluated;
//   * cvRound(t * 255) as  fl(fl(t * 255) + 1.5 * 2^23): the sum is rounded to an integer, ties to even, exactly like cvRound
//     of the rounded product, and the integer sits in the low byte of the float's bit pattern;
//   * the sector's channel assignment is ONE byte permute with a selector looked up by sector (`sel`, kHsvSelectors in LDS)
//     instead of nine selects: sources are byte 0 = q/t, byte 1 = V (one dword) and byte 4 = p (the other);
//   * the interpolation factor x = odd sector ? h : 1 - h, h = (h6 & 255) / 256: with t = h6 & 511 it is |t - 256| / 256
//     (odd sectors have t >= 256; 1 - h is exact).  as_float(0x47000000 | t) is 2^15 + t / 256 (the last place of a
//     float in [2^15, 2^16) is 1 / 256), subtracting 2^15 + 1 is exact, and the absolute value is a source modifier of
//     the product s x: no compare, no select, no convert.
// Proven equal as well, measured, and left out because they did not pay (profiles/r12a_chain_hue_forms.md): S / 255 and
// V / 255 as `or` + fma on 2^23 + n, V into byte 1 through the rounding constant, the channel choice of rgb2hsv_full as
// sign masks + v_bitop3_b32.
// h8: the hue, 0..255.  Returns r | g << 8 | b << 16.
//   sector table (b, g, r): 0 (p, t, V) 1 (p, V, q) 2 (t, V, p) 3 (V, q, p) 4 (V, p, t) 5 (q, p, V)
VKX_COLOR_TABLE uint32_t kHsvSelectors[8] = {0x0c040001u, 0x0c040100u, 0x0c000104u, 0x0c010004u,
                                             0x0c010400u, 0x0c000401u, 0x0c0c0c0cu, 0x0c0c0c0cu};

VKX_COLOR_FN uint32_t hsv2rgb_packed(const uint32_t *sel, uint32_t h8, int S, int V)
{
    const uint32_t h6 = hc::umul24(h8, 6u);                       // h = H * 6 / 256 exactly: sector h6 >> 8, fraction h6 & 255
    const float s = (float)S * (1.0f / 255.0f);
    const float fv = (float)V * (1.0f / 255.0f);
    const float d = hc::u2f(0x47000000u | (h6 & 511u)) - 32769.0f;     // (t - 256) / 256
    const float t1 = fv * (1.f - s);
    const float tt = fv * (1.f - s * hc::abs(d));
    const float m1 = t1 * 255.0f + 12582912.0f;                   // products and sums round separately (-ffp-contract=off)
    const float mt = tt * 255.0f + 12582912.0f;
    const uint32_t lo = hc::f2u(mt) | ((uint32_t)V << 8);         // byte 0 = q / t, byte 1 = V (bits 8..15 of mt are 0)
    return hc::perm(hc::f2u(m1), lo, sel[hc::table_index((int)(h6 >> 8))]);
}

// The hue shift of the fused chain kernel and of the single-stage colour shift: rgb2hsv_full, H + delta modulo 256 (python's
// modulo: delta & 255 is in 0..255 for a negative delta too, and it rides on the rounding term of the hue product),
// hsv2rgb_packed.  Returns r | g << 8 | b << 16.
VKX_COLOR_FN uint32_t hue_shift_packed(const int *sdiv, const int *hdiv, const uint32_t *sel, int delta, int r, int g, int b)
{
    int H, S, V;
    rgb2hsv_full<true>(sdiv, hdiv, r, g, b, H, S, V, (1 << 11) + ((delta & 255) << 12));
    return hsv2rgb_packed(sel, (uint32_t)H & 255u, S, V);
}

} // namespace vkd

#endif // VKX_COLOR_H_
