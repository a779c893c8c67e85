// Host-side check of vkp::Raster (vkit_amd/csrc/vkx_poly_raster.h): seeded random contours, degenerate ones included, go through
// reserve() / add() as the three call sites use them, and the edge and item tables are checked against their invariants.  Plain
// host code: it needs no device.  Build with the sanitizers and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/poly_raster_check.hip -o /tmp/poly_raster_check && /tmp/poly_raster_check
#include "../vkit_amd/csrc/vkx_poly_raster.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>

void vkx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

struct Contour {
    std::vector<int32_t> pts;
    int tag, target, y_lo, y_hi, dx, dy;
    size_t edge_begin, item_begin, item_end;
};

template <int kCross> static void run(unsigned seed, int n_contours)
{
    std::mt19937 rng(seed);
    auto pick = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    std::vector<Contour> contours((size_t)n_contours);
    long long total = 0;
    bool want_overflow = false;
    for (int c = 0; c < n_contours; c++) {
        Contour &C = contours[c];
        const int kind = c % 8;
        int n = pick(3, 12);
        if (kind == 0) n = 1;
        if (kind == 1) n = 2;
        if (kind == 5) n = kCross + pick(-1, 1);        // around the capacity: only kCross + 1 may overflow
        if (kind == 6) n = pick(kCross + 1, 2 * kCross + 40);
        const int flat_y = pick(0, 300);
        for (int i = 0; i < n; i++) {
            int x = pick(-20, 400), y = kind == 2 ? flat_y : pick(-20, 300);   // kind 2: all horizontal
            if (kind == 3 && i > 0 && i % 2) { x = C.pts[2 * (i - 1)]; y = C.pts[2 * (i - 1) + 1]; }   // kind 3: duplicate vertices
            C.pts.push_back(x);
            C.pts.push_back(y);
        }
        C.tag = pick(1, 1 << 20);
        C.target = pick(0, 7);
        const bool band = c % 3 == 0, box = c % 3 == 1;  // a paint band (moved down, clipped to it), a region box (moved up-left), neither
        C.dx = box ? -pick(0, 50) : 0;
        C.dy = band ? C.target * 200 : box ? -pick(0, 50) : 0;
        C.y_lo = band ? C.dy : INT_MIN;
        C.y_hi = band ? C.dy + 200 : INT_MAX;
        total += n;
        want_overflow = want_overflow || n > kCross;
    }
    vkp::Raster<kCross> raster;
    CHECK(!raster.reserve(0x3fffffff) && !raster.reserve(-1));
    CHECK(raster.reserve(total));
    for (Contour &C : contours) {
        C.edge_begin = raster.edges.size();
        C.item_begin = raster.items.size();
        CHECK(raster.add(C.pts.data(), (int)C.pts.size() / 2, C.tag, C.target, C.y_lo, C.y_hi, C.dx, C.dy));
        C.item_end = raster.items.size();
    }
    CHECK(raster.edges.size() == (size_t)total);
    CHECK(raster.may_overflow == want_overflow);

    long long steps = 0;
    for (const Contour &C : contours) {
        const int n = (int)C.pts.size() / 2;
        int ymin = INT_MAX, ymax = INT_MIN;
        for (int i = 0; i < n; i++) {
            const vkp::PolyEdge &e = raster.edges[C.edge_begin + i];
            const int a = (i + n - 1) % n;
            const int xa = C.pts[2 * a] + C.dx, ya = C.pts[2 * a + 1] + C.dy, xb = C.pts[2 * i] + C.dx, yb = C.pts[2 * i + 1] + C.dy;
            CHECK(e.step_base == steps);                 // the prefix sum of dmaj + 1
            steps += e.dmaj + 1;
            CHECK(e.poly == C.tag && e.pad == C.target);
            CHECK(e.dmaj == std::max(std::abs(xb - xa), std::abs(yb - ya)) && e.dmin == std::min(std::abs(xb - xa), std::abs(yb - ya)));
            CHECK(e.lx == std::min(xa, xb) && (e.ly == ya || e.ly == yb));
            CHECK(e.y0 == std::min(ya, yb) && e.y1 == std::max(ya, yb));
            if (ya != yb) {
                ymin = std::min(ymin, e.y0); ymax = std::max(ymax, e.y1);
                CHECK(e.x0_fix == (long long)(ya < yb ? xa : xb) * 65536);
                const long long end = e.x0_fix + (long long)(e.y1 - e.y0) * e.dx_fix, want = (long long)(ya < yb ? xb : xa) * 65536;
                CHECK(std::llabs(end - want) < e.y1 - e.y0);     // the truncated slope misses the far end by less than one unit a row
            }
        }
        // one item a scanline of [ymin, ymax) inside [y_lo, y_hi), each with the contour's edge range, tag and target
        const int lo = std::max(ymin, C.y_lo), hi = std::min(ymax, C.y_hi);
        CHECK(C.item_end - C.item_begin == (size_t)std::max(0LL, (long long)hi - lo));
        for (size_t k = C.item_begin; k < C.item_end; k++) {
            const vkp::Item &it = raster.items[k];
            CHECK(it.edge_begin == (int)C.edge_begin && it.edge_end == (int)C.edge_begin + n);
            CHECK(it.y == lo + (int)(k - C.item_begin) && it.y >= ymin && it.y < ymax && it.y >= C.y_lo && it.y < C.y_hi);
            CHECK(it.tag == C.tag && it.target == C.target);
        }
    }
    CHECK(steps == raster.steps);
}

int main()
{
    for (unsigned seed = 0; seed < 40; seed++) {
        run<vkp::kPaintCross>(seed, 1 + (int)(seed * 7 % 60));
        run<vkp::kPolyCross>(seed, 1 + (int)(seed % 9));
    }
    {   // outlines too long: two edges of 2^30 steps each
        vkp::Raster<64> raster;
        const int32_t pts[4] = {0, 0, 0x3fffffff, 0};
        CHECK(raster.reserve(4));
        CHECK(!raster.add(pts, 2, 1, 0));
    }
    printf("poly raster host check ok\n");
    return 0;
}
