// vkit_amd/csrc/vkx_tile_bins.h on its own, on the CPU: the CSR tile bins against a brute-force test of every (tile, item) pair,
// their bound, and the per-box tile prefix.  Plain C++17; tests/test_tile_bins.py builds it with and without sanitizers.
// Prints one line '<check>: 0 of N mismatches' per check and 'all checks hold' at the end; exit status 1 otherwise.
#include "../vkit_amd/csrc/vkx_tile_bins.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()      // splitmix64, high word
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
int uniform(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }      // inclusive

struct Rect { int up, down, left, right; };

long long failures = 0;
void report(const char *name, long long bad, long long n)
{
    printf("%s: %lld of %lld mismatches\n", name, bad, n);
    failures += bad;
}

struct Tally { long long cases = 0, start0 = 0, monotone = 0, total = 0, lists = 0; };

// one random case on TW x TH tiles; `widen`: the span of the rectangle grown by a reach and clamped, as the combiner's is;
// `sieve`: a keep predicate that drops about a third of the pairs and every pair of some tiles
template <int TW, int TH>
void one_case(Tally &tally, bool widen, bool sieve)
{
    const int h = rnd() % 4 == 0 ? uniform(1, 9) : uniform(1, 300), w = rnd() % 4 == 0 ? uniform(1, 33) : uniform(1, 300);
    const int n = rnd() % 8 == 0 ? 0 : uniform(0, 200), reach = widen ? uniform(0, 70) : 0;
    std::vector<Rect> rects((size_t)n);
    for (Rect &r : rects) {
        const bool small = rnd() % 2;
        r.up = uniform(0, h - 1);
        r.down = std::min(h - 1, r.up + (small ? uniform(0, 2 * TH) : uniform(0, h - 1)));
        r.left = uniform(0, w - 1);
        r.right = std::min(w - 1, r.left + (small ? uniform(0, 2 * TW) : uniform(0, w - 1)));
        if (rnd() % 16 == 0) { r.up -= r.up % TH; r.left -= r.left % TW; }      // on a tile border
    }
    const uint32_t salt = rnd();
    auto kept = [&](size_t t, int i) { return !sieve || (t % 5 != 3 && (t * 31 + (size_t)i * 17 + salt) % 3 != 0); };
    auto grown = [&](const Rect &r) {
        return Rect{std::max(0, r.up - reach), std::min(h - 1, r.down + reach), std::max(0, r.left - reach), std::min(w - 1, r.right + reach)};
    };

    vkb::TileBins<TW, TH> bins(h, w);
    auto span_of = [&](int i) {
        const Rect g = grown(rects[i]);
        return bins.rect(g.up, g.down, g.left, g.right);
    };
    std::vector<int> list;
    bool counted;
    if (sieve) counted = bins.count(n, 1ll << 30, span_of, kept);
    else counted = bins.count(n, 1ll << 30, span_of);
    if (counted) {
        list.assign(bins.pairs() + 1, -7);       // one guard entry behind the last
        if (sieve) bins.fill(n, list.data(), span_of, kept);
        else bins.fill(n, list.data(), span_of);
    }

    tally.cases++;
    const size_t n_tiles = (size_t)((w + TW - 1) / TW) * ((h + TH - 1) / TH);
    if (!counted || bins.n_tiles() != n_tiles || bins.start.size() != n_tiles + 1) {
        tally.start0++; tally.monotone++; tally.total++; tally.lists++;
        return;
    }
    if (bins.start[0] != 0) tally.start0++;
    bool mono = true;
    for (size_t t = 0; t < n_tiles; t++) mono = mono && bins.start[t] <= bins.start[t + 1];
    if (!mono) tally.monotone++;
    // brute force: tile t meets item i when their pixel rectangles intersect
    std::vector<int> want;
    std::vector<size_t> want_start(1, 0);
    const int tiles_x = (w + TW - 1) / TW;
    for (size_t t = 0; t < n_tiles; t++) {
        const int ty = (int)(t / tiles_x), tx = (int)(t % tiles_x);
        const Rect tile{ty * TH, ty * TH + TH - 1, tx * TW, tx * TW + TW - 1};
        for (int i = 0; i < n; i++) {
            const Rect g = grown(rects[i]);
            if (g.up <= tile.down && tile.up <= g.down && g.left <= tile.right && tile.left <= g.right && kept(t, i)) want.push_back(i);
        }
        want_start.push_back(want.size());
    }
    if (!mono || (size_t)bins.start[n_tiles] != want.size() || bins.pairs() != want.size() || list.back() != -7) {
        tally.total++; tally.lists++;
        return;
    }
    bool same = true;
    for (size_t t = 0; t <= n_tiles; t++) same = same && (size_t)bins.start[t] == want_start[t];
    same = same && std::equal(want.begin(), want.end(), list.begin());
    if (!same) tally.lists++;
}

template <int TW, int TH>
void shape_cases(Tally &tally, int n_cases)
{
    for (int c = 0; c < n_cases; c++) one_case<TW, TH>(tally, c % 3 == 1, c % 4 >= 2);
}

// the bound: `bound` kept pairs pass, one more is refused, and the refused pass saw bound + 1 kept pairs, not all of them
void bound_checks()
{
    long long bad_pass = 0, bad_refuse = 0, bad_visits = 0, n = 0;
    for (int round = 0; round < 40; round++) {
        const int h = uniform(8, 120), w = uniform(32, 300), n_items = uniform(1, 60);
        vkb::TileBins<32, 8> bins(h, w);
        const bool sieve = round % 2;
        long long kept_calls = 0;
        auto span_of = [&](int) { return bins.rect(0, h - 1, 0, w - 1); };       // every item meets every tile
        auto kept = [&](size_t t, int i) {
            const bool k = !sieve || (t + (size_t)i) % 2 == 0;
            kept_calls += k;
            return k;
        };
        if (!bins.count(n_items, 1ll << 30, span_of, kept)) { bad_pass++; n++; continue; }
        const long long pairs = (long long)bins.pairs();
        n++;
        if (pairs != kept_calls || pairs < 1) { bad_pass++; continue; }
        kept_calls = 0;
        if (!bins.count(n_items, pairs, span_of, kept) || (long long)bins.pairs() != pairs) bad_pass++;
        kept_calls = 0;
        if (bins.count(n_items, pairs - 1, span_of, kept)) bad_refuse++;
        if (kept_calls > pairs) bad_visits++;                                   // pairs = (bound) + 1
        // far more pairs than the bound: still bound + 1
        const long long small = std::min<long long>(pairs - 1, 3);
        kept_calls = 0;
        if (bins.count(n_items, small, span_of, kept)) bad_refuse++;
        if (kept_calls != small + 1) bad_visits++;
    }
    report("bound: exactly the bound is taken", bad_pass, n);
    report("bound: one pair more is refused", bad_refuse, 2 * n);
    report("bound: a refused pass stops at the pair beyond the bound", bad_visits, 2 * n);
}

template <int TW, int TH>
void prefix_cases(long long &bad, long long &n_checked)
{
    for (int c = 0; c < 200; c++) {
        const int n = c % 10 == 0 ? 0 : uniform(0, 200);
        std::vector<long long> bh((size_t)n), bw((size_t)n);
        for (int i = 0; i < n; i++) { bh[i] = uniform(1, 5 * TH + 1); bw[i] = uniform(1, 5 * TW + 1); }
        std::vector<int> starts(3, -1);
        const bool ok = vkb::box_tile_starts<TW, TH>(n, [&](int i, long long &h, long long &w) { h = bh[i]; w = bw[i]; }, starts);
        bool same = ok && starts.size() == (size_t)n + 1;
        long long sum = 0;
        for (int i = 0; same && i <= n; i++) {
            same = starts[i] == sum;
            if (i < n) {
                long long tiles = 0;         // a direct count: the tile origins inside the box
                for (long long y = 0; y < bh[i]; y += TH)
                    for (long long x = 0; x < bw[i]; x += TW) tiles++;
                sum += tiles;
            }
        }
        bad += !same;
        n_checked++;
    }
}

void prefix_checks()
{
    long long bad = 0, n = 0;
    prefix_cases<16, 16>(bad, n);
    prefix_cases<32, 8>(bad, n);
    report("box prefix: starts equal the direct sums", bad, n);

    // 2^31 tiles from synthetic sides (nothing is allocated per tile): 2^31 - 1 is taken, 2^31 is refused
    bad = 0;
    std::vector<int> starts;
    const long long side = 1ll << 15;       // 2^11 x 2^11 tiles of 16 x 16: 2^22 tiles a box
    auto full = [&](int, long long &h, long long &w) { h = side; w = side; };
    if (!vkb::box_tile_starts<16, 16>(511, full, starts) || starts[511] != 511 * (1 << 22)) bad++;
    if (vkb::box_tile_starts<16, 16>(512, full, starts)) bad++;
    // ... and exactly at the edge: 511 such boxes, then one of 2^22 - 1 tiles (taken) or 2^22 tiles (refused)
    auto edge = [&](long long last_w) {
        return [=](int i, long long &h, long long &w) { h = i < 511 ? side : 16; w = i < 511 ? side : last_w; };
    };
    if (!vkb::box_tile_starts<16, 16>(512, edge(16ll * ((1 << 22) - 1)), starts) || starts[512] != 0x7fffffff) bad++;
    if (vkb::box_tile_starts<16, 16>(512, edge(16ll * (1 << 22)), starts)) bad++;
    if (vkb::box_tile_starts<16, 16>(512, edge(16ll * ((1 << 22) - 1) + 1), starts)) bad++;
    report("box prefix: refused at 2^31 tiles", bad, 5);
}

}  // namespace

int main()
{
    Tally tally;
    shape_cases<32, 8>(tally, 400);
    shape_cases<32, 32>(tally, 400);
    shape_cases<64, 16>(tally, 400);
    report("bins: start[0] is 0", tally.start0, tally.cases);
    report("bins: start is monotone", tally.monotone, tally.cases);
    report("bins: start[n_tiles] is the length of the list", tally.total, tally.cases);
    report("bins: every tile lists its kept items in ascending order", tally.lists, tally.cases);
    bound_checks();
    prefix_checks();
    if (failures) {
        printf("%lld checks failed\n", failures);
        return 1;
    }
    printf("all checks hold\n");
    return 0;
}
