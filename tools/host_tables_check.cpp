// The process-wide host tables of vkit_amd/csrc/vkx_host_tables.h, entered from eight threads at once and checked against a
// plain reference (tests/test_host_tables_threads.py).  The header is all this program includes of the library.  Build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -o host_tables_check tools/host_tables_check.cpp     (the race check)
//   g++ -O2 -std=c++17 -pthread -o host_tables_check tools/host_tables_check.cpp                          (the values)
//
// Eight threads spin on one atomic counter until all have arrived, then each makes its FIRST call to both accessors -- the even
// threads SinTable first, the odd ones the jump tables -- and checksums every byte it reads.  After the join the main thread
// checks, one line each:
//   checksums     the eight threads read the same bytes
//   sin bound     |table[d] - sin(d pi / 180)| <= 5e-8 + 2^-24 for d = 0 .. 450 (a 7-decimal literal, rounded to float32)
//   sin exact     table[0] == 0, table[90] == table[450] == 1, table[270] == -1
//   lane, a64/g64, a128/g128, pow2[0..20]
//                 A_j s + inc G_j against the generator stepped one draw at a time, s <- A s + inc (mod 2^128), from two
//                 (state, inc) pairs; A is PCG64's multiplier as written out below, not the header's
//   pow2[21..63]  the doubling identities A_2j = A_j^2, G_2j = G_j (A_j + 1)
// Exit status 0: every check holds.  The first mismatches of a check are printed.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>

#include "../vkit_amd/csrc/vkx_host_tables.h"

typedef unsigned __int128 u128;

static const int kThreads = 8;
static std::atomic<int> g_arrived{0};
static uint64_t g_sum[kThreads];

static uint64_t fnv1a(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

static void worker(int t)
{
    g_arrived.fetch_add(1);
    while (g_arrived.load() < kThreads) {}
    const float *sn = nullptr;
    const vkx_host_tables::JumpTabs *jt = nullptr;
    if (t & 1) { jt = &vkx_host_tables::jump_tabs(); sn = vkx_host_tables::sin_table(); }
    else { sn = vkx_host_tables::sin_table(); jt = &vkx_host_tables::jump_tabs(); }
    uint64_t h = 0xCBF29CE484222325ull;
    h = fnv1a(h, sn, 451 * sizeof(float));
    h = fnv1a(h, jt, sizeof *jt);
    g_sum[t] = h;
}

static u128 mk(const uint64_t *w) { return ((u128)w[1] << 64) | w[0]; }
static u128 mk(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }

static int g_failed = 0;

static void report(const char *name, int bad, int of)
{
    printf("%s: %d of %d mismatch%s\n", name, bad, of, bad == 1 ? "" : "es");
    if (bad) g_failed++;
}

int main()
{
    std::thread th[kThreads];
    for (int t = 0; t < kThreads; t++) th[t] = std::thread(worker, t);
    for (int t = 0; t < kThreads; t++) th[t].join();

    int bad = 0;
    for (int t = 1; t < kThreads; t++)
        if (g_sum[t] != g_sum[0]) {
            bad++;
            printf("  thread %d read %016llx, thread 0 %016llx\n", t, (unsigned long long)g_sum[t], (unsigned long long)g_sum[0]);
        }
    report("checksums of 8 threads", bad, kThreads - 1);

    // ---- SinTable against sin itself
    const float *sn = vkx_host_tables::sin_table();
    const double bound = 5e-8 + 0x1p-24;
    bad = 0;
    for (int d = 0; d <= 450; d++) {
        const double want = sin((double)d * 3.14159265358979323846 / 180.0), err = fabs((double)sn[d] - want);
        if (!(err <= bound)) {
            if (bad++ < 8) printf("  table[%d] = %.9g, sin = %.17g, error %.3g > %.3g\n", d, (double)sn[d], want, err, bound);
        }
    }
    report("sin bound, d = 0 .. 450", bad, 451);
    bad = 0;
    const struct { int d; float v; } exact[] = {{0, 0.0f}, {90, 1.0f}, {450, 1.0f}, {270, -1.0f}};
    for (const auto &e : exact)
        if (!(sn[e.d] == e.v)) {
            bad++;
            printf("  table[%d] = %.9g, not %g\n", e.d, (double)sn[e.d], (double)e.v);
        }
    report("sin exact at 0, 90, 270, 450", bad, 4);

    // ---- the jump tables against the generator stepped one draw at a time
    const vkx_host_tables::JumpTabs &jt = vkx_host_tables::jump_tabs();
    const u128 A = mk(0x2360ED051FC65DA4ull, 0x4385DF649FCCF645ull);       // PCG64's multiplier (pcg64.h: PCG_DEFAULT_MULTIPLIER_128)
    const struct { u128 state, inc; } pairs[2] = {
        {mk(0x0123456789ABCDEFull, 0xFEDCBA9876543210ull), mk(0x9E3779B97F4A7C15ull, 0xF39CC0605CEDC835ull)},
        {mk(0xD1B54A32D192ED03ull, 0x8CB92BA72F3D8DD7ull), mk(0x5851F42D4C957F2Dull, 0x14057B7EF767814Full)},
    };
    int bad_lane = 0, bad_64 = 0, bad_128 = 0, bad_pow2 = 0;
    for (int p = 0; p < 2; p++) {
        const u128 s0 = pairs[p].state, inc = pairs[p].inc;
        u128 s = s0;
        for (uint64_t j = 1; j <= (1ull << 20); j++) {
            s = A * s + inc;
            if (j <= 64 && mk(&jt.lane[j - 1][0]) * s0 + inc * mk(&jt.lane[j - 1][2]) != s) {
                if (bad_lane++ < 8) printf("  pair %d: lane[%d] does not jump %d draws\n", p, (int)j - 1, (int)j);
            }
            if (j == 64 && mk(jt.a64) * s0 + inc * mk(jt.g64) != s) {
                bad_64++;
                printf("  pair %d: a64 / g64 do not jump 64 draws\n", p);
            }
            if (j == 128 && mk(jt.a128) * s0 + inc * mk(jt.g128) != s) {
                bad_128++;
                printf("  pair %d: a128 / g128 do not jump 128 draws\n", p);
            }
            if ((j & (j - 1)) == 0) {
                int i = 0;
                while ((1ull << i) < j) i++;
                if (mk(&jt.pow2[i][0]) * s0 + inc * mk(&jt.pow2[i][2]) != s) {
                    if (bad_pow2++ < 8) printf("  pair %d: pow2[%d] does not jump 2^%d draws\n", p, i, i);
                }
            }
        }
    }
    report("lane[l] against j = 1 .. 64 single steps, 2 pairs", bad_lane, 128);
    report("a64 / g64 against 64 single steps, 2 pairs", bad_64, 2);
    report("a128 / g128 against 128 single steps, 2 pairs", bad_128, 2);
    report("pow2[0 .. 20] against 2^i single steps, 2 pairs", bad_pow2, 42);
    bad = 0;
    for (int i = 21; i < 64; i++) {
        const u128 a = mk(&jt.pow2[i - 1][0]), g = mk(&jt.pow2[i - 1][2]);
        if (mk(&jt.pow2[i][0]) != a * a || mk(&jt.pow2[i][2]) != g * (a + 1)) {
            if (bad++ < 8) printf("  pow2[%d] is not pow2[%d] doubled\n", i, i - 1);
        }
    }
    report("pow2[21 .. 63] doubling identities", bad, 43);

    if (g_failed) printf("FAILED: %d check(s)\n", g_failed);
    else printf("all checks hold\n");
    return g_failed ? 1 : 0;
}
