// The host-side axis tables of cv.resize that resize.hip builds (and defines), declared for the batched glyph resize of
// seal_fill.hip: each table stated once, bit for bit oracle/vkx_oracle.c's.
#pragma once
#include "vkx_resize_cubic.h"

#include <vector>

namespace vkd {

struct AxisTable8 {
    std::vector<int> ofs;
    std::vector<float> coef;   // [n][8]
    std::vector<short> icoef;
};

struct AreaTab {
    std::vector<int> start;    // [dsize + 1] first entry of every destination index
    std::vector<int> si;
    std::vector<float> alpha;
};

void build_axis8(int ssize, int dsize, AxisTable8 *t);      // LANCZOS4: 8 taps from s - 3
void build_linear_exact_axis(int ssize, int dsize, std::vector<int> *ofs, std::vector<int> *w1, int *dmin, int *dmax);
void build_area_tab(int ssize, int dsize, double scale, AreaTab *t);

} // namespace vkd
