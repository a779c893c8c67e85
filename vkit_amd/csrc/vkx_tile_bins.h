// Items binned into the tiles of a plane, on the host: the CSR tables the tile kernels walk (quad_interp.hip, region_label.hip,
// image_combine.hip) and the per-box tile prefix of the kernels that take one workgroup per tile of a box (char_mask.hip,
// char_heatmap.hip; vkd::box_tile_pixel decodes it).  Plain C++17, no HIP include: tools/tile_bins_check.cpp compiles this header
// alone and checks it against a brute-force test of every (tile, item) pair (tests/test_tile_bins.py).
#pragma once

#include <cstddef>
#include <vector>

namespace vkb {

// The tiles an item meets: columns tx0 .. tx1 of rows ty0 .. ty1, both inclusive.
struct TileSpan {
    int tx0, tx1, ty0, ty1;
};

struct KeepAll {
    bool operator()(size_t, int) const { return true; }
};

// CSR bins of n items over the TW x TH tiles of an h x w plane, h, w >= 1.  count() makes `start` (n_tiles() + 1 entries: tile t
// lists start[t] .. start[t + 1]), fill() writes the item indices, ascending inside every tile, where the caller wants them -- a
// vector, or the staged block itself.  span_of(i) is the TileSpan of item i; keep(tile, i) drops a pair (the same answers in
// both passes).
template <int TW, int TH>
struct TileBins {
    int tiles_x, tiles_y;
    std::vector<int> start;

    TileBins(int h, int w) : tiles_x((w + TW - 1) / TW), tiles_y((h + TH - 1) / TH) {}
    size_t n_tiles() const { return (size_t)tiles_x * tiles_y; }
    size_t pairs() const { return (size_t)start.back(); }

    // the span of rows up .. down, columns left .. right (inclusive, inside the plane)
    static TileSpan rect(int up, int down, int left, int right) { return TileSpan{left / TW, right / TW, up / TH, down / TH}; }

    // False: more than max_pairs (< 2^31) kept pairs.  The pass ends AT the first pair beyond the bound: a refused call has cost
    // max_pairs + 1 kept pairs, however many the items would have made.
    template <class SpanOf, class Keep = KeepAll>
    bool count(int n, long long max_pairs, SpanOf span_of, Keep keep = Keep())
    {
        start.assign(n_tiles() + 1, 0);
        long long total = 0;
        for (int i = 0; i < n; i++) {
            const TileSpan s = span_of(i);
            for (int ty = s.ty0; ty <= s.ty1; ty++)
                for (int tx = s.tx0; tx <= s.tx1; tx++) {
                    const size_t t = (size_t)ty * tiles_x + tx;
                    if (!keep(t, i)) continue;
                    if (++total > max_pairs) return false;
                    start[t + 1]++;
                }
        }
        for (size_t t = 0; t < n_tiles(); t++) start[t + 1] += start[t];
        return true;
    }

    // after count(): list[0 .. pairs())
    template <class SpanOf, class Keep = KeepAll>
    void fill(int n, int *list, SpanOf span_of, Keep keep = Keep()) const
    {
        std::vector<int> cursor(start.begin(), start.end() - 1);
        for (int i = 0; i < n; i++) {
            const TileSpan s = span_of(i);
            for (int ty = s.ty0; ty <= s.ty1; ty++)
                for (int tx = s.tx0; tx <= s.tx1; tx++) {
                    const size_t t = (size_t)ty * tiles_x + tx;
                    if (keep(t, i)) list[cursor[t]++] = i;
                }
        }
    }
};

// The tile prefix of n boxes, each laid out as ceil(bh / TH) * ceil(bw / TW) tiles of its own: box i owns tiles starts[i] ..
// starts[i + 1].  size_of(i, bh, bw) gives the sides of box i.  False: 2^31 tiles or more.
template <int TW, int TH, class SizeOf>
bool box_tile_starts(int n, SizeOf size_of, std::vector<int> &starts)
{
    starts.resize((size_t)n + 1);
    long long tiles = 0;
    for (int i = 0; i < n; i++) {
        long long bh, bw;
        size_of(i, bh, bw);
        starts[i] = (int)tiles;
        tiles += ((bh + TH - 1) / TH) * ((bw + TW - 1) / TW);
        if (tiles >= (1LL << 31)) return false;
    }
    starts[n] = (int)tiles;
    return true;
}

} // namespace vkb
