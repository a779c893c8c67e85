// Exhaustive check of the cheaper forms in vkit_amd/csrc/vkx_color.h, on the host (tests/test_hue_forms_exhaustive.py).
// The header compiles without HIP; its device builtins have plain C++ fallbacks, so this program runs the source lines the
// kernels compile.  Build:  g++ -O2 -std=c++17 -ffp-contract=off -o hue_forms_check tools/hue_forms_check.cpp
//
//   hue_forms_check forward             all 2^24 (r, g, b): S, V and H mod 256 of rgb2hsv_full (both WRAP_H forms, and the
//                                       hue with a shift riding on the rounding term) against the plain integer arithmetic
//                                       of oracle/vkx_oracle.c, restated below
//   hue_forms_check backward            all 2^24 (H, S, V): hsv2rgb_packed against hsv2rgb_full's r | g << 8 | b << 16
//   hue_forms_check roundtrip D FILE    hue_shift_packed with delta D over the all-triples image (pixel i = (i >> 16,
//                                       (i >> 8) & 255, i & 255)), written to FILE as 2^24 RGB triples: the test compares
//                                       it with the oracle's color_shift_rgb
// Exit status 0: no mismatch.  The first mismatches are printed.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../vkit_amd/csrc/vkx_color.h"

static int g_sdiv[256], g_hdiv[256];

static void init_tables()
{
    // cvRound of a double: round to nearest, ties to even
    g_sdiv[0] = g_hdiv[0] = 0;
    for (int i = 1; i < 256; i++) {
        g_sdiv[i] = (int)nearbyint((255 << 12) / (1. * i));
        g_hdiv[i] = (int)nearbyint((256 << 12) / (6. * i));
    }
}

// RGB -> HSV_FULL as the oracle states it: compares, masks, full 32-bit products.
static void ref_rgb2hsv(int r, int g, int b, int &H, int &S, int &V)
{
    int v = b, vmin = b;
    if (g > v) v = g;
    if (r > v) v = r;
    if (g < vmin) vmin = g;
    if (r < vmin) vmin = r;
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    S = (diff * g_sdiv[v] + (1 << 11)) >> 12;
    int hh = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    hh = (hh * g_hdiv[diff] + (1 << 11)) >> 12;
    hh += hh < 0 ? 256 : 0;
    H = hh;
    V = v;
}

static long report(const char *what, long bad, unsigned i, long got, long want)
{
    if (bad < 8) printf("%s: triple %06x: got %lx, want %lx\n", what, i, (unsigned long)got, (unsigned long)want);
    return bad + 1;
}

static int forward()
{
    long bad = 0;
    for (unsigned i = 0; i < (1u << 24); i++) {
        const int r = i >> 16, g = (i >> 8) & 255, b = i & 255;
        int H0, S0, V0, H, S, V;
        ref_rgb2hsv(r, g, b, H0, S0, V0);
        if (H0 < 0 || H0 > 255 || S0 < 0 || S0 > 255) bad = report("reference out of range", bad, i, H0, S0);
        vkd::rgb2hsv_full<false>(g_sdiv, g_hdiv, r, g, b, H, S, V);
        if (H != H0 || S != S0 || V != V0) bad = report("rgb2hsv_full<false>", bad, i, H << 16 | S << 8 | V, H0 << 16 | S0 << 8 | V0);
        vkd::rgb2hsv_full<true>(g_sdiv, g_hdiv, r, g, b, H, S, V);
        if ((H & 255) != H0 || S != S0 || V != V0) bad = report("rgb2hsv_full<true>", bad, i, (H & 255) << 16 | S << 8 | V, H0 << 16 | S0 << 8 | V0);
        // the shift on the rounding term, as hue_shift_packed passes it: four shifts on every triple, every shift on one
        // triple in 251 (the round trip at the test's deltas covers the path end to end)
        for (int k = 0; k < 256; k += (i % 251) ? 85 : 1) {
            vkd::rgb2hsv_full<true>(g_sdiv, g_hdiv, r, g, b, H, S, V, (1 << 11) + (k << 12));
            if ((H & 255) != ((H0 + k) & 255) || S != S0 || V != V0) bad = report("rgb2hsv_full<true> + shift", bad, i, H & 255, (H0 + k) & 255);
        }
    }
    printf("forward: %ld mismatches\n", bad);
    return bad != 0;
}

static int backward()
{
    long bad = 0;
    for (unsigned i = 0; i < (1u << 24); i++) {
        const int H = i >> 16, S = (i >> 8) & 255, V = i & 255;
        int r, g, b;
        vkd::hsv2rgb_full(H, S, V, r, g, b);
        const uint32_t want = (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16;
        if ((unsigned)r > 255u || (unsigned)g > 255u || (unsigned)b > 255u) bad = report("hsv2rgb_full out of range", bad, i, want, 0);
        const uint32_t got = vkd::hsv2rgb_packed(vkd::kHsvSelectors, (uint32_t)H, S, V);
        if (got != want) bad = report("hsv2rgb_packed", bad, i, got, want);
    }
    printf("backward: %ld mismatches\n", bad);
    return bad != 0;
}

static int roundtrip(int delta, const char *path)
{
    std::vector<unsigned char> out((size_t)3 << 24);
    for (unsigned i = 0; i < (1u << 24); i++) {
        const uint32_t p = vkd::hue_shift_packed(g_sdiv, g_hdiv, vkd::kHsvSelectors, delta, i >> 16, (i >> 8) & 255, i & 255);
        out[3 * (size_t)i] = (unsigned char)p;
        out[3 * (size_t)i + 1] = (unsigned char)(p >> 8);
        out[3 * (size_t)i + 2] = (unsigned char)(p >> 16);
        if (p >> 24) { printf("roundtrip: triple %06x: byte 3 is not zero (%08x)\n", i, p); return 1; }
    }
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) { printf("cannot write %s\n", path); return 2; }
    return 0;
}

int main(int argc, char **argv)
{
    init_tables();
    if (argc == 2 && !strcmp(argv[1], "forward")) return forward();
    if (argc == 2 && !strcmp(argv[1], "backward")) return backward();
    if (argc == 4 && !strcmp(argv[1], "roundtrip")) return roundtrip(atoi(argv[2]), argv[3]);
    fprintf(stderr, "usage: %s forward | backward | roundtrip DELTA FILE\n", argv[0]);
    return 2;
}
