// The lossy half of libjpeg-turbo's baseline encoder, shared by the round trip (jpeg.hip) and the encoder (jpeg_encode.hip):
// the quantisation tables of a quality, the 16-bit fixed-point colour conversion and one pass of the accurate integer forward
// DCT (CONST_BITS 13, PASS1_BITS 2).  tests/jpeg_restate.py is the statement the goldens pin.
#pragma once
#include "vkx_internal.h"

namespace vkx_jpeg {

// quantisation of one quality: the table entries and exact reciprocals of 8q (n * m >> 32 == n / 8q for n < 2^21)
struct JpegTables {
    int q[2][64];           // [0] luma, [1] chroma; natural order
    unsigned m[2][64];      // ceil(2^32 / 8q)
};

constexpr int C_0_298 = 2446, C_0_390 = 3196, C_0_541 = 4433, C_0_765 = 6270;
constexpr int C_0_899 = 7373, C_1_175 = 9633, C_1_501 = 12299, C_1_847 = 15137;
constexpr int C_1_961 = 16069, C_2_053 = 16819, C_2_562 = 20995, C_3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the forward DCT over d[0..7]; `last`: the column pass (descale by PASS1_BITS, not scale up)
template <bool last>
__device__ __forceinline__ void fdct8(int *d)
{
    constexpr int sh = last ? 13 + 2 : 13 - 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7];
    const int t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5];
    const int t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = last ? descale(t10 + t11, 2) : (t10 + t11) * 4;
    d[4] = last ? descale(t10 - t11, 2) : (t10 - t11) * 4;
    const int z1e = (t12 + t13) * C_0_541;
    d[2] = descale(z1e + t13 * C_0_765, sh);
    d[6] = descale(z1e - t12 * C_1_847, sh);
    const int z5 = (t4 + t6 + t5 + t7) * C_1_175;
    const int z1 = -(t4 + t7) * C_0_899, z2 = -(t5 + t6) * C_2_562;
    const int z3 = -(t4 + t6) * C_1_961 + z5, z4 = -(t5 + t7) * C_0_390 + z5;
    d[7] = descale(t4 * C_0_298 + z1 + z3, sh);
    d[5] = descale(t5 * C_2_053 + z2 + z4, sh);
    d[3] = descale(t6 * C_3_072 + z2 + z3, sh);
    d[1] = descale(t7 * C_1_501 + z1 + z4, sh);
}

__device__ __forceinline__ int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// Annex K.1 / K.2, natural order
constexpr int kStdLuma[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr int kStdChroma[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jpeg_set_quality(quality, force_baseline = TRUE); quality 0 scales as 1
inline JpegTables jpeg_tables(int quality)
{
    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    const long scale = q < 50 ? 5000 / q : 200 - 2 * q;
    JpegTables t;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            long v = ((c ? kStdChroma : kStdLuma)[i] * scale + 50) / 100;
            v = v < 1 ? 1 : v > 255 ? 255 : v;
            t.q[c][i] = (int)v;
            const unsigned long long div = 8ull * (unsigned long long)v;
            t.m[c][i] = (unsigned)(((1ull << 32) + div - 1) / div);
        }
    return t;
}

} // namespace vkx_jpeg
