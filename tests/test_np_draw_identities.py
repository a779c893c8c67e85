"""The identities phase 1 of the numpy-stream draw pass rests on (csrc/nprand.hip, walk_tile), checked exactly and without a GPU.

  value   fma(2^52 + rabs, wi, -2^52 wi), the sign put on the result, against (2^52 + rabs - 2^52) * (+-wi): a host C program built with
          -ffp-contract=off compares the bits for all 256 layers, both signs, rabs in {0, 1, ki - 1, ki, 2^52 - 1} and 10^5 random ones
          per layer, and the rounded step of five deviations with the sign on the value and with the sign on the scale
  fields  rotr64(x, r + 9) holds rabs, the layer and the sign where the kernel takes them, against the extraction from rotr64(x, r)
  stride  the limb-wise step s -> a s + c of the kernel, restated here, against (a s + c) mod 2^128 on limbs of all zeros, all ones, ..."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1

C_SOURCE = r'''
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "np_ziggurat.h"
static double b2d(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t d2b(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static uint64_t rs = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
int main(void)
{
    const double scales[5] = {0.5, 1.0, 10.0, 37.5, 300.0};
    const uint64_t m52 = (1ull << 52) - 1;
    unsigned long long bad_c = 0, bad_x = 0, bad_step = 0, bad_scale_form = 0, n = 0;
    for (int idx = 0; idx < 256; idx++) {
        const double wi = b2d(kNpZigW[idx]);
        const double c = -4503599627370496.0 * wi;
        /* c is exact: dividing the power of two out again gives wi, and both are normal */
        if (!(c / -4503599627370496.0 == wi && fpclassify(wi) == FP_NORMAL && fpclassify(c) == FP_NORMAL && wi > 0.0)) bad_c++;
        for (int k = 0; k < 100005; k++) {
            uint64_t rabs;
            switch (k) {
            case 0: rabs = 0; break;
            case 1: rabs = 1; break;
            case 2: rabs = (kNpZigK[idx] - 1) & m52; break;
            case 3: rabs = kNpZigK[idx] & m52; break;
            case 4: rabs = m52; break;
            default: rabs = rnd() & m52;
            }
            const double D = b2d(0x4330000000000000ull | rabs);
            for (int sign = 0; sign < 2; sign++, n++) {
                const uint64_t sbit = (uint64_t)sign << 63;
                const double x_old = (D - 4503599627370496.0) * b2d(kNpZigW[idx] | sbit);
                const double xa = fma(D, wi, c);
                const double x_new = b2d(d2b(xa) | sbit);
                if (d2b(x_old) != d2b(x_new)) bad_x++;
                for (int s = 0; s < 5; s++) {
                    const uint64_t want = d2b(scales[s] * x_old + 6755399441055744.0);
                    if (d2b(scales[s] * x_new + 6755399441055744.0) != want) bad_step++;
                    if (d2b(b2d(d2b(scales[s]) | sbit) * xa + 6755399441055744.0) != want) bad_scale_form++;
                }
            }
        }
    }
    printf("%llu %llu %llu %llu %llu\n", n, bad_c, bad_x, bad_step, bad_scale_form);
    return 0;
}
'''


def test_one_fma_gives_the_bits_of_subtract_and_multiply(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'a host C compiler builds the oracle; this test needs it too'
    src = tmp_path / 'np_fma_identity.c'
    src.write_text(C_SOURCE)
    exe = tmp_path / 'np_fma_identity'
    subprocess.run([cc, '-O2', '-ffp-contract=off', '-I', os.path.join(ROOT, 'vkit_amd', 'csrc'), '-o', str(exe), str(src), '-lm'], check=True)
    n, bad_c, bad_x, bad_step, bad_scale_form = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert n == 256 * 2 * 100_005
    assert (bad_c, bad_x, bad_step, bad_scale_form) == (0, 0, 0, 0)


def _rotr64(x, n):
    n &= 63
    return ((x >> n) | (x << (64 - n))) & M64


def test_one_rotation_by_r_plus_9_holds_every_field():
    rnd = random.Random(5)
    xs = [0, M64, 1, 1 << 63, 0xffffffff00000000, 0x00000000ffffffff] + [rnd.getrandbits(64) for _ in range(300)]
    for r in range(64):
        for x in xs:
            u = _rotr64(x, r)                      # today's word: idx = bits 0-7, sign = bit 8, rabs = bits 9-60
            idx, sign, rabs = u & 0xff, (u >> 8) & 1, (u >> 9) & ((1 << 52) - 1)
            # the kernel's form: x >> ((r + 9) & 63) | x << ((55 - r) & 63), each shift taking its amount modulo 64
            v = ((x >> ((r + 9) & 63)) | (x << ((55 - r) & 63))) & M64
            assert v == _rotr64(x, r + 9)
            lo, hi = v & M32, v >> 32
            assert lo == rabs & M32                                         # the low word of 2^52 + rabs as it is
            assert (hi & 0x000fffff) | 0x43300000 == 0x43300000 | (rabs >> 32)   # its high word: one and-or
            assert hi >> 31 == sign                                         # the sign in bit 31 of the high word
            assert (hi >> 19) & 0xff0 == 16 * idx                           # the byte offset of the 16-byte table entry


def _limbs(v, n):
    return [(v >> (32 * i)) & M32 for i in range(n)]


def _addc(a, b, c):
    t = a + b + c
    return t & M32, t >> 32


def _lcg_step_limbwise(s, a, c):
    """lcg_step of csrc/nprand.hip: 64-bit column accumulators that cannot overflow or may wrap, and two carry chains of three over
    32-bit halves -- [F.hi : F.lo : E.hi] + [G.lo : O1.hi : O1.lo], then + [H.lo : O2.hi : O2.lo]."""
    s0, s1, s2, s3 = _limbs(s, 4)
    a0, a1, a2, a3 = _limbs(a, 4)
    c0, c1, c23 = c & M32, (c >> 32) & M32, c >> 64
    E = a0 * s0 + c0
    O1 = a0 * s1 + c1
    O2 = a1 * s0
    assert E <= M64 and O1 <= M64 and O2 <= M64            # a 32 x 32 product plus a 32-bit addend fits 64 bits
    F = (a0 * s2 + c23 + a1 * s1 + a2 * s0) & M64          # bits 64 .. 127: wraps
    G = (a0 * s3 + a1 * s2) & M32                          # bits 96 .. 127: low words
    H = (a2 * s1 + a3 * s0) & M32
    t, ca = _addc(E >> 32, O1 & M32, 0)
    u, cc = _addc(F & M32, O1 >> 32, ca)
    w, _ = _addc(F >> 32, G, cc)
    r1, cb = _addc(t, O2 & M32, 0)
    r2, cd = _addc(u, O2 >> 32, cb)
    r3, _ = _addc(w, H, cd)
    return (r3 << 96) | (r2 << 64) | (r1 << 32) | (E & M32)


def test_limbwise_stride_step_is_the_128_bit_multiply_add():
    pats = (0, M32, 1, 0x80000000)
    values = [sum(l << (32 * i) for i, l in enumerate(ls)) for ls in itertools.product(pats, repeat=4)]
    assert 0 in values and M128 in values and M64 in values and 0xffffffff00000000ffffffff00000000 in values
    a128 = pow(0x2360ED051FC65DA44385DF649FCCF645, 128, 1 << 128)     # the multiplier of a 128-draw stride
    rnd = random.Random(9)
    mults = [a128, M128, 1, 0xffffffff00000000ffffffff00000001, 0x00000000ffffffff00000000ffffffff] + [rnd.getrandbits(128) | 1 for _ in range(8)]
    adds = [0, 1, M128, 0xffffffff00000000ffffffff00000001, M64, rnd.getrandbits(128) | 1]
    for a in mults:
        for c in adds:
            for s in values:
                assert _lcg_step_limbwise(s, a, c) == (a * s + c) & M128, (hex(s), hex(a), hex(c))
    for _ in range(20_000):
        s, a, c = rnd.getrandbits(128), rnd.getrandbits(128), rnd.getrandbits(128)
        assert _lcg_step_limbwise(s, a, c) == (a * s + c) & M128
