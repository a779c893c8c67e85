// Host-side check of the resize plan and table blocks (vkit_amd/csrc/vkx_resize_axes.h): a seeded sweep of geometries, sides
// 1 .. 300, both dtypes, every interpolation code and some unknown ones, the exact-half and integer-factor cases among them,
// goes through vkd::plan_resize and the packers as resize.hip, seal_fill.hip and region_flatten.hip use them; every block is
// written between guard bytes and read back through its view.  Every geometry also goes, with the five codes of the batched
// sites on both dtypes and one job of equal shapes, through ONE vkd::ResizePlanner as seal_fill.hip and text_line.hip drive it
// (plan, layout, pack): between guard bytes each block must be, byte for byte, what the direct packer writes.  Plain host code: it
// needs no device.  Build with the sanitizers and run (and once more plain, at -O2):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/resize_tables_check.hip -o /tmp/resize_tables_check && /tmp/resize_tables_check
#include "../vkit_amd/csrc/vkx_resize_axes.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

static char last_error[256];                    // what the library keeps for vkx_last_error
void vkx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

static long long n_plans, n_refused, n_nan_rows, n_blocks[3], n_modes[vkd::M_REFUSED_UNKNOWN + 1];
static long long n_planner_jobs, n_planner_blocks, n_planner_refused;

// a block of exactly `bytes` between two guards: pack(nullptr) announced the size, pack(address) must fill it and no more
struct Guarded {
    static constexpr size_t kGuard = 64;
    std::vector<unsigned char> mem;
    size_t bytes;
    explicit Guarded(size_t n) : mem(n + 2 * kGuard, 0xa5), bytes(n) {}
    unsigned char *block() { return mem.data() + kGuard; }
    void check_guards() const
    {
        for (size_t i = 0; i < kGuard; i++) CHECK(mem[i] == 0xa5 && mem[kGuard + bytes + i] == 0xa5);
    }
    // the last byte a view's table reaches is the block's last byte or before it
    void holds(const void *first, size_t n) const
    {
        CHECK((const unsigned char *)first >= mem.data() + kGuard && (const unsigned char *)first + n <= mem.data() + kGuard + bytes);
    }
};

template <class CT>
static void check_taps(int ks, int sh, int sw, int dh, int dw)
{
    const bool f32 = sizeof(CT) == sizeof(float);
    Guarded g(vkd::pack_taps(ks, f32, sh, sw, dh, dw, nullptr));
    std::vector<int> yofs_host;
    CHECK(vkd::pack_taps(ks, f32, sh, sw, dh, dw, g.block(), &yofs_host) == g.bytes);
    g.check_guards();
    const vkd::TapView<CT> t(g.block(), ks, dh, dw);
    g.holds(t.xofs, sizeof(int) * dw); g.holds(t.yofs, sizeof(int) * dh);
    g.holds(t.xcoef, sizeof(CT) * ks * dw); g.holds(t.ycoef, sizeof(CT) * ks * dh);
    CHECK((const unsigned char *)(t.ycoef + (size_t)ks * dh) == g.block() + g.bytes);       // the four tables fill the block
    CHECK(yofs_host.size() == (size_t)dh && std::equal(yofs_host.begin(), yofs_host.end(), t.yofs));
    // Offsets: floor((d + 0.5) * scale - 0.5) lies in [-1, size - 1] (the kernels clip every tap s - left .. s + ks / 2 to the
    // source); the horizontal 2-tap table is pinned into the source, its column is read unclipped.  They ascend, which the
    // separable tiles of resize.hip plan on.
    for (int x = 0; x < dw; x++) {
        CHECK(t.xofs[x] >= (ks == 2 ? 0 : -1) && t.xofs[x] <= sw - 1);
        CHECK(x == 0 || t.xofs[x] >= t.xofs[x - 1]);
    }
    for (int y = 0; y < dh; y++) {
        CHECK(t.yofs[y] >= -1 && t.yofs[y] <= sh - 1);
        CHECK(y == 0 || t.yofs[y] >= t.yofs[y - 1]);
    }
    // Coefficients, a row of ks at a time: an ordinary row has a sum of |a| below 2^12 (below 2 in float), which keeps the
    // horizontal sum of taps_pixel_u8 below 255 * 2^12 < 2^20; the only other row is the NaN column of LANCZOS4, one tap NaN
    // (-32768 in fixed point) and the others 0, where it stays below 255 * 2^15 < 2^23 -- the bound its 24-bit multiply states.
    const CT *coef[2] = {t.xcoef, t.ycoef};
    const int rows[2] = {dw, dh};
    for (int a = 0; a < 2; a++)
        for (int d = 0; d < rows[a]; d++) {
            const CT *c = coef[a] + (size_t)ks * d;
            double sum = 0;
            int bad = 0, zeros = 0;
            for (int k = 0; k < ks; k++) {
                const bool odd = f32 ? c[k] != c[k] : c[k] == (CT)-32768;
                bad += odd;
                zeros += c[k] == 0;
                if (!odd) sum += c[k] < 0 ? -(double)c[k] : (double)c[k];
            }
            if (bad) { CHECK(ks == 8 && bad == 1 && zeros == ks - 1); n_nan_rows++; }
            else CHECK(sum < (f32 ? 2.0 : 4096.0));
        }
    n_blocks[0]++;
}

static void check_linear_exact(int sh, int sw, int dh, int dw)
{
    int range[4] = {-7, -7, -7, -7};
    Guarded g(vkd::pack_linear_exact(sh, sw, dh, dw, nullptr, range));
    CHECK(range[0] == -7);                                  // sizing writes nothing
    CHECK(vkd::pack_linear_exact(sh, sw, dh, dw, g.block(), range) == g.bytes);
    g.check_guards();
    const vkd::LinearExactView t = vkd::LinearExactView::of(g.block(), dh, dw);
    g.holds(t.xofs, sizeof(int) * dw); g.holds(t.xw, sizeof(int) * dw); g.holds(t.yofs, sizeof(int) * dh); g.holds(t.yw, sizeof(int) * dh);
    CHECK((const unsigned char *)(t.yw + dh) == g.block() + g.bytes);
    const int *ofs[2] = {t.xofs, t.yofs}, *w[2] = {t.xw, t.yw}, dsize[2] = {dw, dh}, ssize[2] = {sw, sh};
    for (int a = 0; a < 2; a++) {
        const int mn = range[2 * a], mx = range[2 * a + 1];
        CHECK(0 <= mn && mn <= mx && mx <= dsize[a]);
        for (int d = 0; d < dsize[a]; d++) {
            CHECK(ofs[a][d] >= 0 && ofs[a][d] < ssize[a] && w[a][d] >= 0 && w[a][d] <= 256);
            if (d >= mn && d < mx) CHECK(ofs[a][d] + 1 < ssize[a]);      // an interpolating index reads ofs and ofs + 1
        }
    }
    n_blocks[1]++;
}

static void check_area(const vkd::ResizePlan &plan, int sh, int sw, int dh, int dw)
{
    const vkd::AreaTabs tabs(sh, sw, dh, dw, plan.scale_x, plan.scale_y);
    Guarded g(tabs.pack(nullptr));
    CHECK(tabs.pack(g.block()) == g.bytes);
    g.check_guards();
    const int nx = (int)tabs.x.si.size(), ny = (int)tabs.y.si.size();
    const vkd::AreaView t(g.block(), dh, dw, nx, ny);
    g.holds(t.xstart, sizeof(int) * (dw + 1)); g.holds(t.ystart, sizeof(int) * (dh + 1));
    g.holds(t.xsi, sizeof(int) * nx); g.holds(t.ysi, sizeof(int) * ny); g.holds(t.xal, sizeof(float) * nx); g.holds(t.yal, sizeof(float) * ny);
    CHECK((const unsigned char *)(t.yal + ny) == g.block() + g.bytes);
    // the counts the device-side view reads out of the block itself
    CHECK(((const int *)g.block())[dw] == nx && ((const int *)g.block())[dw + 1 + dh] == ny);
    const int *start[2] = {t.xstart, t.ystart}, *si[2] = {t.xsi, t.ysi}, dsize[2] = {dw, dh}, ssize[2] = {sw, sh}, n[2] = {nx, ny};
    const float *al[2] = {t.xal, t.yal};
    for (int a = 0; a < 2; a++) {
        CHECK(start[a][0] == 0 && start[a][dsize[a]] == n[a]);
        for (int d = 0; d < dsize[a]; d++) {
            CHECK(start[a][d] < start[a][d + 1]);           // contiguous, non-empty runs
            double sum = 0;
            for (int k = start[a][d]; k < start[a][d + 1]; k++) {
                CHECK(si[a][k] >= 0 && si[a][k] < ssize[a]);
                CHECK(k == start[a][d] || si[a][k] == si[a][k - 1] + 1);
                CHECK(al[a][k] > 0.f && al[a][k] <= 1.f);
                sum += al[a][k];
            }
            CHECK(sum > 0.99 && sum < 1.01);
        }
    }
    n_blocks[2]++;
}

static void run(bool f32, int code, int sh, int sw, int dh, int dw)
{
    const vkd::ResizePlan plan = vkd::plan_resize(f32, code, sh, sw, dh, dw);
    const bool known = code >= VKX_INTER_NEAREST && code <= VKX_INTER_NEAREST_EXACT;
    const bool half = sw == 2 * dw && sh == 2 * dh;
    // AREA itself, and the float32 2 x 2 shrink that cv.resize hands to AREA (never an enlargement)
    const bool area = code == VKX_INTER_AREA || (f32 && half && (code == VKX_INTER_LINEAR || code == VKX_INTER_LINEAR_EXACT));
    n_plans++;
    n_modes[plan.mode]++;
    CHECK(plan.mode != vkd::M_COPY);
    CHECK(plan.refused() == (!known || (area && (dw > sw || dh > sh))));
    CHECK((plan.mode == vkd::M_REFUSED_UNKNOWN) == !known);
    if (plan.refused()) { n_refused++; return; }
    CHECK(plan.scale_x == 1. / ((double)dw / sw) && plan.scale_y == 1. / ((double)dh / sh));
    switch (plan.mode) {
    case vkd::M_NEAREST: CHECK(code == VKX_INTER_NEAREST); break;
    case vkd::M_NEAREST_EXACT:
        CHECK(code == VKX_INTER_NEAREST_EXACT);
        // the kernels take min(index, size - 1): the first index of an axis is not negative and the indices ascend
        CHECK(plan.p[0] > 0 && plan.p[1] >= 0 && plan.p[2] > 0 && plan.p[3] >= 0);
        break;
    case vkd::M_TAPS:
        CHECK((code == VKX_INTER_CUBIC && plan.ks == 4) || (code == VKX_INTER_LANCZOS4 && plan.ks == 8));
        if (f32) check_taps<float>(plan.ks, sh, sw, dh, dw); else check_taps<short>(plan.ks, sh, sw, dh, dw);
        break;
    case vkd::M_LINEAR_U8: CHECK(!f32 && code == VKX_INTER_LINEAR && !half); check_taps<short>(2, sh, sw, dh, dw); break;
    case vkd::M_LINEAR_F32: CHECK(f32 && !half && (code == VKX_INTER_LINEAR || code == VKX_INTER_LINEAR_EXACT)); break;
    case vkd::M_LINEAR_EXACT_U8: CHECK(!f32 && code == VKX_INTER_LINEAR_EXACT && !half); check_linear_exact(sh, sw, dh, dw); break;
    case vkd::M_HALF_U8: CHECK(!f32 && half && (code == VKX_INTER_LINEAR || code == VKX_INTER_LINEAR_EXACT)); break;
    case vkd::M_AREA_FAST:
        CHECK(area && plan.p[0] * dw == sw && plan.p[1] * dh == sh);        // the box of the last pixel ends with the source
        break;
    case vkd::M_AREA:
        CHECK(area);
        check_area(plan, sh, sw, dh, dw);
        break;
    default: CHECK(!"a mode plan_resize does not return");
    }
}

// One planner over every (dtype, code) of the batched sites at this geometry, and one job of equal shapes: what the two entry
// points do with the resizes of a call.  The blocks lie between guard bytes at the offsets layout() was given.
static void check_planner(int sh, int sw, int dh, int dw)
{
    constexpr size_t kGuard = 64;
    const int codes[5] = {VKX_INTER_CUBIC, VKX_INTER_AREA, VKX_INTER_LANCZOS4, VKX_INTER_LINEAR_EXACT, VKX_INTER_NEAREST_EXACT};
    struct Job { vkd::PlannedResize r; bool f32; int code; bool planned; };
    std::vector<Job> jobs;                      // (sized before the first plan(): the planner keeps the jobs' addresses)
    for (int code : codes)
        for (int f32 = 0; f32 < 2; f32++) jobs.push_back(Job{{}, f32 != 0, code, false});
    jobs.push_back(Job{{}, false, VKX_INTER_AREA, false});                       // equal shapes, below
    vkd::ResizePlanner planner("check_planner");
    for (int code = -1; code <= 8; code++) {
        bool known = false;
        for (int c : codes) known = known || c == code;
        CHECK(vkd::ResizePlanner::known_interpolation(code) == known);
    }
    for (size_t k = 0; k < jobs.size(); k++) {
        Job &j = jobs[k];
        const bool equal = k + 1 == jobs.size();
        const int th = equal ? sh : dh, tw = equal ? sw : dw;
        last_error[0] = 0;
        const int rc = planner.plan(j.r, j.f32, j.code, sh, sw, th, tw);
        CHECK(j.r.sh == sh && j.r.sw == sw && j.r.dh == th && j.r.dw == tw && j.r.tab_off == 0);
        if (sh == th && sw == tw) {             // nothing is resized: nothing is planned, whatever the code
            CHECK(rc == VKX_OK && j.r.plan.mode == vkd::M_COPY);
            continue;
        }
        const vkd::ResizePlan direct = vkd::plan_resize(j.f32, j.code, sh, sw, th, tw);
        CHECK(direct.mode != vkd::M_REFUSED_UNKNOWN);
        if (direct.refused()) {                 // an enlarging AREA
            CHECK(j.code == VKX_INTER_AREA && (tw > sw || th > sh));
            CHECK(rc == VKX_ERR_INVALID && std::string(last_error) == "check_planner: requirement failed: INTER_AREA is for shrinking only");
            n_planner_refused++;
            continue;
        }
        CHECK(rc == VKX_OK && last_error[0] == 0 && j.r.plan.mode == direct.mode && j.r.plan.ks == direct.ks);
        j.planned = true;
        n_planner_jobs++;
    }
    // the layout: every block behind a guard of its own
    size_t end = kGuard, asked = 0;
    planner.layout([&](size_t bytes) { CHECK(bytes > 0); const size_t off = end; end = off + bytes + kGuard; asked++; return off; });
    std::vector<unsigned char> got(end, 0xa5), want(end, 0xa5);
    planner.pack(got.data());
    // what the direct packers write, at the same offsets
    size_t blocks = 0;
    for (Job &j : jobs) {
        if (!j.planned) { CHECK(j.r.tab_off == 0); continue; }
        const vkd::ResizePlan direct = vkd::plan_resize(j.f32, j.code, sh, sw, dh, dw);
        unsigned char *at = want.data() + j.r.tab_off;
        int range[4] = {0, 0, 0, 0};
        size_t bytes = 0;
        switch (direct.mode) {
        case vkd::M_TAPS: bytes = vkd::pack_taps(direct.ks, j.f32, sh, sw, dh, dw, nullptr); break;
        case vkd::M_LINEAR_EXACT_U8: bytes = vkd::pack_linear_exact(sh, sw, dh, dw, nullptr, range); break;
        case vkd::M_AREA: bytes = vkd::AreaTabs(sh, sw, dh, dw, direct.scale_x, direct.scale_y).pack(nullptr); break;
        default: break;
        }
        if (!bytes) { CHECK(j.r.tab_off == 0); continue; }
        CHECK(j.r.tab_off >= (long long)kGuard && (size_t)j.r.tab_off + bytes + kGuard <= end);
        switch (direct.mode) {
        case vkd::M_TAPS: vkd::pack_taps(direct.ks, j.f32, sh, sw, dh, dw, at); break;
        case vkd::M_LINEAR_EXACT_U8: vkd::pack_linear_exact(sh, sw, dh, dw, at, range); break;
        default: vkd::AreaTabs(sh, sw, dh, dw, direct.scale_x, direct.scale_y).pack(at); break;
        }
        blocks++;
        // the plan as the record carries it to the device: a LINEAR_EXACT job holds its ranges once it is packed
        for (int i = 0; i < 4; i++) CHECK(j.r.plan.p[i] == (direct.mode == vkd::M_LINEAR_EXACT_U8 ? range[i] : direct.p[i]));
        CHECK(j.r.plan.scale_x == direct.scale_x && j.r.plan.scale_y == direct.scale_y);
    }
    CHECK(blocks == asked);
    CHECK(got == want);                         // every block and every guard byte
    n_planner_blocks += (long long)blocks;
}

int main()
{
    std::mt19937 rng(20240607u);
    auto pick = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    const int codes[] = {0, 1, 2, 3, 4, 5, 6, -1, 7, 100};
    for (int round = 0; round < 1500; round++) {
        int sh = pick(1, 300), sw = pick(1, 300), dh = pick(1, 300), dw = pick(1, 300);
        switch (round % 8) {
        case 1: dh = pick(1, 150); dw = pick(1, 150); sh = 2 * dh; sw = 2 * dw; break;                  // the exact half
        case 2: dh = pick(1, 60); dw = pick(1, 60); sh = dh * pick(1, 5); sw = dw * pick(1, 5); break;   // integer factors
        case 3: sh = pick(1, 300); sw = pick(1, 300); dh = pick(1, sh); dw = pick(1, sw); break;         // a shrink on both axes
        case 4: sw = 1; break;
        case 5: sh = 1; break;
        case 6: dh = pick(1, 3); dw = pick(1, 3); break;
        case 7: sh = pick(1, 8); sw = pick(1, 8); break;                                               // large enlargements
        default: break;
        }
        for (int code : codes)
            for (int f32 = 0; f32 < 2; f32++) run(f32 != 0, code, sh, sw, dh, dw);
        check_planner(sh, sw, dh, dw);
    }
    // the geometries of the NaN LANCZOS4 coefficient column (one tap saturates to -32768, the others are 0)
    const int nan_geometries[3][4] = {{146, 4, 64, 196}, {127, 1, 202, 197}, {4, 146, 196, 64}};
    for (const auto &g : nan_geometries)
        for (int f32 = 0; f32 < 2; f32++) {
            const long long before = n_nan_rows;
            run(f32 != 0, VKX_INTER_LANCZOS4, g[0], g[1], g[2], g[3]);
            CHECK(n_nan_rows > before);
        }
    for (int m = vkd::M_NEAREST; m <= vkd::M_REFUSED_UNKNOWN; m++) CHECK(n_modes[m] > 0);
    CHECK(n_blocks[0] > 0 && n_blocks[1] > 0 && n_blocks[2] > 0);
    CHECK(n_planner_jobs > 0 && n_planner_blocks > 0 && n_planner_refused > 0);
    printf("resize planner host check ok: %lld jobs planned, %lld refused, %lld blocks equal to the direct packers'\n", n_planner_jobs,
           n_planner_refused, n_planner_blocks);
    printf("resize tables host check ok: %lld plans (%lld refused), %lld tap, %lld linear-exact and %lld area blocks\n", n_plans, n_refused,
           n_blocks[0], n_blocks[1], n_blocks[2]);
    return 0;
}
