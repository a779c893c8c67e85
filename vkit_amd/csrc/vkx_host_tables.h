// The two process-wide host tables of the library: OpenCV's SinTable (ellipse.hip) and the PCG64 jump constants (nprand.hip).
// Contexts of several threads reach them together -- one vkx_ctx per thread is the contract, and a thread pool's first calls
// arrive at once -- so each is a function-local `static const` object built by its constructor and read-only afterwards.
// Plain C++17, no HIP include: tools/host_tables_check.cpp compiles this header alone and enters it from eight threads under
// ThreadSanitizer (tests/test_host_tables_threads.py).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace vkx_host_tables {

typedef unsigned __int128 u128;

// ---- OpenCV's SinTable: sin of whole degrees 0 .. 450 as float literals with seven decimals ---------------------------------

struct SinTable {
    float v[451];
    SinTable()
    {
        for (int d = 0; d <= 450; d++) {
            char text[32];
            snprintf(text, sizeof text, "%.7f", std::sin((double)d * 3.14159265358979323846 / 180.0));
            v[d] = strtof(text, nullptr);
        }
    }
};

// Built by the first caller; the language makes every other thread wait for the constructor (a function-local static).
inline const float *sin_table()
{
    static const SinTable table;
    return table.v;
}

// ---- PCG64's stream-independent jump constants ---------------------------------------------------------------------------------

#define VKX_PCG_MULT ((((vkx_host_tables::u128)0x2360ED051FC65DA4ull) << 64) | (vkx_host_tables::u128)0x4385DF649FCCF645ull)

// s_{k + j} = A^j s_k + inc * G_j with G_j = 1 + A + ... + A^(j-1) (mod 2^128).
struct JumpTabs {
    uint64_t pow2[64][4];    // j = 2^i: A^j lo, hi, G_j lo, hi
    uint64_t lane[64][4];    // j = l + 1
    uint64_t a64[2], g64[2];
    uint64_t a128[2], g128[2];
};

inline void jump_consts(u128 j, u128 *a, u128 *g)
{
    u128 acc_mult = 1, acc_plus = 0, cur_mult = VKX_PCG_MULT, cur_plus = 1;
    while (j > 0) {
        if (j & 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        j >>= 1;
    }
    *a = acc_mult;
    *g = acc_plus;
}

struct JumpTabsBuilt {
    JumpTabs t;
    JumpTabsBuilt()
    {
        auto put = [](uint64_t *w, u128 a, u128 g) {
            w[0] = (uint64_t)a; w[1] = (uint64_t)(a >> 64); w[2] = (uint64_t)g; w[3] = (uint64_t)(g >> 64);
        };
        u128 a, g;
        for (int i = 0; i < 64; i++) { jump_consts((u128)1 << i, &a, &g); put(t.pow2[i], a, g); }
        for (int l = 0; l < 64; l++) { jump_consts((u128)(l + 1), &a, &g); put(t.lane[l], a, g); }
        jump_consts(64, &a, &g);
        t.a64[0] = (uint64_t)a; t.a64[1] = (uint64_t)(a >> 64);
        t.g64[0] = (uint64_t)g; t.g64[1] = (uint64_t)(g >> 64);
        jump_consts(128, &a, &g);
        t.a128[0] = (uint64_t)a; t.a128[1] = (uint64_t)(a >> 64);
        t.g128[0] = (uint64_t)g; t.g128[1] = (uint64_t)(g >> 64);
    }
};

// JumpTabs itself stays a plain struct: the kernels read a copy of it (NpTabs::jump).  Built as SinTable is.
inline const JumpTabs &jump_tabs()
{
    static const JumpTabsBuilt built;
    return built.t;
}

} // namespace vkx_host_tables
