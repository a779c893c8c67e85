// The small layers PageAssemblerStep composites besides text on gfx950: non-text symbols (reference:
// vkit/pipeline/text_detection/page_non_text_symbol.py:107-169 after engine/image/selector.py:98-101), the score maps of the two
// barcode engines (engine/barcode/qr.py:81-93, code39.py:137-148) and the text-line bounding-box frames
// (pipeline/text_detection/page_text_line_bounding_box.py:94-147).
//
// A page has a dozen symbols, a few barcodes and a few frames of tens to a few hundred pixels a side.  Composed from the
// single-plane operations every item is a resize launch, a download and host numpy; here one call takes EVERY such layer of a
// page, its records, resize tables and host sources staged as one block (vkx_tables, one copy out of the ring), in at most TWO
// launches and without a synchronisation:
//   k_layer_symbols  one lane a pixel of a symbol: the pixel of vkx_resize_pixel.h its plan names (INTER_CUBIC, or the copy of equal
//                    shapes).  An RGBA symbol stores its image and leaves float32(a) in its alpha plane, the workgroup's largest a
//                    going to the record's maximum with ONE integer atomic (exact); a grayscale symbol stores its constant colour
//                    and its finished alpha plane, (g > 0) * float32(alpha).
//   k_layer_planes   one lane a pixel of a float plane: an RGBA symbol's ((a / 255) * alpha) / (max / 255), four float32 roundings
//                    (max == 0: 0 / 0, NaN throughout, as numpy has it); a barcode's module mask as mask ? alpha : 0, resized
//                    (INTER_CUBIC) and clipped to [0, 1] unless it has the box's shape already; a frame's ring of alpha around 0,
//                    seen through its trim window.
// A call without RGBA symbols has no maxima to wait for; one without symbols is the second launch alone.  The maxima travel
// zeroed inside the staged block, so nothing clears them on the device.  A 64 x 4 tile a workgroup, as the sibling record kernels
// have it: the records are far smaller than the device, so the grid is as many small workgroups as the pixels give, none holds
// LDS beyond the four partial maxima, and the per-record fields are uniform over a workgroup (scalar loads).
#include "vkx_internal.h"
#include "vkx_resize_pixel.h"
#include "vkx_tile_bins.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

namespace {

constexpr int kMaxLayers = 4096;
constexpr int kMaxSide = 32767;

struct LayerRec {
    int kind;                                   // VKX_LAYER_*
    int oh, ow;                                 // the planes written
    int color[3];                               // SYMBOL_GRAY
    float alpha;
    int box_h, box_w, thick, trim_up, trim_left;   // FRAME: the untrimmed plane, its ring, where the window starts
    const uint8_t *src;                         // dense [sh][sw][4 RGBA, else 1]
    uint8_t *img;                               // symbols: uint8 [oh][ow][3]
    float *pln;                                 // float32 [oh][ow]
    vkd::PlannedResize r;
};

// the layer of a workgroup of either grid and the workgroup's 64 x 4 tile of it: `which` lists the layers of the grid, `starts`
// their tile prefix (vkb::box_tile_starts)
__device__ __forceinline__ int layer_tile_pixel(const LayerRec *recs, const int *which, const int *starts, int n, int &x, int &y)
{
    return which[vkd::box_tile_pixel<64, 4>(n, starts, [&](int i) { return recs[which[i]].ow; }, x, y)];
}

__global__ void __launch_bounds__(256) k_layer_symbols(const LayerRec *__restrict__ recs, const int *__restrict__ which,
                                                       const int *__restrict__ starts, int n, const unsigned char *__restrict__ tabs,
                                                       unsigned *__restrict__ rec_max)
{
    __shared__ unsigned part[4];
    int x, y;
    const int li = layer_tile_pixel(recs, which, starts, n, x, y);
    const LayerRec &L = recs[li];
    const bool live = x < L.ow && y < L.oh;
    const uint8_t *src = L.src;
    const int sw = L.r.sw;
    if (L.kind == VKX_LAYER_SYMBOL_GRAY) {
        if (!live) return;
        uint8_t g;
        vkd::planned_pixel_u8<1>(L.r, tabs, y, x, [&](int yy, int b) { return (int)src[(ptrdiff_t)yy * sw + b]; }, &g);
        const ptrdiff_t at = (ptrdiff_t)y * L.ow + x;
        uint8_t *o = L.img + 3 * at;
        o[0] = (uint8_t)L.color[0]; o[1] = (uint8_t)L.color[1]; o[2] = (uint8_t)L.color[2];
        L.pln[at] = g > 0 ? L.alpha : 0.f;      // (mat > 0).astype(np.float32) * alpha
        return;
    }
    unsigned a = 0u;
    if (live) {
        uint8_t px[4];
        vkd::planned_pixel_u8<4>(L.r, tabs, y, x, [&](int yy, int b) { return (int)src[(ptrdiff_t)yy * 4 * sw + b]; }, px);
        const ptrdiff_t at = (ptrdiff_t)y * L.ow + x;
        uint8_t *o = L.img + 3 * at;
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
        a = px[3];
        L.pln[at] = (float)a;                   // k_layer_planes finishes it in place
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = max(a, (unsigned)__shfl_xor((int)a, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned top = max(max(part[0], part[1]), max(part[2], part[3]));
        if (top) atomicMax(rec_max + li, top);
    }
}

__global__ void __launch_bounds__(256) k_layer_planes(const LayerRec *__restrict__ recs, const int *__restrict__ which,
                                                      const int *__restrict__ starts, int n, const unsigned char *__restrict__ tabs,
                                                      const unsigned *__restrict__ rec_max)
{
    int x, y;
    const int li = layer_tile_pixel(recs, which, starts, n, x, y);
    const LayerRec &L = recs[li];
    if (x >= L.ow || y >= L.oh) return;
    float *p = L.pln + (ptrdiff_t)y * L.ow + x;
    if (L.kind == VKX_LAYER_SYMBOL_RGBA) {      // np_alpha = a.astype(float32) / 255; np_alpha *= alpha; np_alpha /= np_alpha.max()
        const float unit = *p / 255.f;
        const float scaled = unit * L.alpha;
        const float top = (float)rec_max[li] / 255.f;
        *p = scaled / top;
    } else if (L.kind == VKX_LAYER_SCORE) {
        const uint8_t *src = L.src;
        const int sw = L.r.sw;
        const float alpha = L.alpha;
        *p = vkd::planned_pixel_f32(L.r, tabs, y, x, [&](int yy, int xx) { return src[(ptrdiff_t)yy * sw + xx] ? alpha : 0.f; });
    } else {                                    // FRAME: ScoreMap.from_shape(value=alpha), the empty box filled with 0.0, the trim window
        const int by = y + L.trim_up, bx = x + L.trim_left;
        const bool inside = by >= L.thick && by < L.box_h - L.thick && bx >= L.thick && bx < L.box_w - L.thick;
        *p = inside ? 0.f : L.alpha;
    }
}

}  // namespace

VKX_EXPORT int vkx_page_layers_dev(vkx_ctx *ctx, const vkx_page_layer *layers_host, int n_layers, const void *blob_host,
                                   size_t blob_bytes, uint8_t *dst, size_t dst_bytes)
{
    VKX_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "1 .. 4096 layers");
    VKX_REQUIRE(ctx && layers_host && dst, "NULL argument");
    VKX_REQUIRE(blob_host || blob_bytes == 0, "NULL blob");
    VKX_REQUIRE(blob_bytes <= ((size_t)1 << 30) && dst_bytes <= ((size_t)1 << 40), "blob beyond 2^30 or dst beyond 2^40 bytes");
    VKX_REQUIRE((uintptr_t)dst % 4 == 0, "dst not aligned to 4 bytes");

    auto side = [](int v) { return v >= 1 && v <= kMaxSide; };
    std::vector<LayerRec> recs(n_layers);
    std::vector<int> sym_which, pln_which, sym_starts, pln_starts;
    std::vector<std::pair<long long, long long>> ranges;
    vkd::ResizePlanner planner(__func__);

    for (int i = 0; i < n_layers; i++) {
        const vkx_page_layer &p = layers_host[i];
        LayerRec &L = recs[i];
        const bool symbol = p.kind == VKX_LAYER_SYMBOL_RGBA || p.kind == VKX_LAYER_SYMBOL_GRAY;
        VKX_REQUIRE(symbol || p.kind == VKX_LAYER_SCORE || p.kind == VKX_LAYER_FRAME, "unknown layer kind");
        VKX_REQUIRE(side(p.src_h) && side(p.src_w) && side(p.out_h) && side(p.out_w), "side outside 1 .. 32767");
        VKX_REQUIRE(p.alpha >= 0.0 && p.alpha <= 1.0, "alpha NaN or outside [0, 1]");
        L.kind = p.kind; L.oh = p.out_h; L.ow = p.out_w; L.alpha = (float)p.alpha;
        for (int c = 0; c < 3; c++) {
            VKX_REQUIRE(p.color[c] >= 0 && p.color[c] <= 255, "colour outside 0 .. 255");
            L.color[c] = p.color[c];
        }
        L.box_h = p.src_h; L.box_w = p.src_w; L.thick = 0; L.trim_up = L.trim_left = 0;
        L.src = nullptr; L.img = nullptr;
        L.r = vkd::PlannedResize{vkd::ResizePlan(), 0, 1, 1, 1, 1};

        if (p.kind == VKX_LAYER_FRAME) {
            // the reference's asserts: empty_box.up < empty_box.down, .left < .right
            VKX_REQUIRE(p.thickness >= 1 && 2 * (long long)p.thickness + 1 < p.src_h && 2 * (long long)p.thickness + 1 < p.src_w,
                        "frame thickness leaves no interior");
            for (int k = 0; k < 4; k++) VKX_REQUIRE(p.trim[k] >= 0 && p.trim[k] <= kMaxSide, "frame trim outside 0 .. 32767");
            VKX_REQUIRE(p.trim[0] + p.trim[1] < p.src_h && p.trim[2] + p.trim[3] < p.src_w, "frame trims leave no window");
            VKX_REQUIRE(p.out_h == p.src_h - p.trim[0] - p.trim[1] && p.out_w == p.src_w - p.trim[2] - p.trim[3],
                        "frame output is not its trim window");
            L.thick = p.thickness; L.trim_up = p.trim[0]; L.trim_left = p.trim[2];
        } else {
            const size_t src_bytes = (size_t)p.src_h * p.src_w * (p.kind == VKX_LAYER_SYMBOL_RGBA ? 4 : 1);
            if (p.src_off >= 0) {
                VKX_REQUIRE((unsigned long long)p.src_off <= blob_bytes && src_bytes <= blob_bytes - (size_t)p.src_off, "source outside the blob");
            } else {
                VKX_REQUIRE(p.src_off == -1 && p.src_dev, "a source is a blob offset, or -1 and a device array");
                VKX_REQUIRE_DISJOINT(p.src_dev, 1, 0, src_bytes, dst, 1, 0, dst_bytes);
                L.src = (const uint8_t *)p.src_dev;
            }
            if (int rc = planner.plan(L.r, p.kind == VKX_LAYER_SCORE, VKX_INTER_CUBIC, p.src_h, p.src_w, p.out_h, p.out_w)) return rc;
        }

        const long long area = (long long)p.out_h * p.out_w;
        VKX_REQUIRE(p.alpha_off >= 0 && p.alpha_off % 4 == 0 && (unsigned long long)(p.alpha_off + 4 * area) <= dst_bytes,
                    "float plane outside dst or not aligned to 4 bytes");
        ranges.emplace_back(p.alpha_off, p.alpha_off + 4 * area);
        L.pln = (float *)(dst + p.alpha_off);
        if (symbol) {
            VKX_REQUIRE(p.image_off >= 0 && (unsigned long long)(p.image_off + 3 * area) <= dst_bytes, "symbol image outside dst");
            ranges.emplace_back(p.image_off, p.image_off + 3 * area);
            L.img = dst + p.image_off;
            sym_which.push_back(i);
        }
        if (p.kind != VKX_LAYER_SYMBOL_GRAY) pln_which.push_back(i);
    }
    VKX_REQUIRE(!vkx_ranges_overlap(ranges), "layer destinations overlap one another");
    const auto starts_of = [&](const std::vector<int> &which, std::vector<int> &starts) {
        return vkb::box_tile_starts<64, 4>((int)which.size(), [&](int k, long long &bh, long long &bw) { bh = recs[which[k]].oh; bw = recs[which[k]].ow; },
                                           starts) && starts.back() < (1 << 30);
    };
    VKX_REQUIRE(starts_of(sym_which, sym_starts) && starts_of(pln_which, pln_starts), "too many pixels for one call");

    // one staged block: records, the two grids' layer lists and tile prefixes, the zeroed maxima, table blocks, the blob
    vkx_tables tab(ctx);
    const size_t recs_off = tab.add(sizeof(LayerRec) * (size_t)n_layers);
    const size_t sym_off = tab.add(sizeof(int) * (sym_which.size() + sym_starts.size()));
    const size_t pln_off = tab.add(sizeof(int) * (pln_which.size() + pln_starts.size()));
    const size_t max_off = tab.add(sizeof(unsigned) * (size_t)n_layers);
    planner.layout([&](size_t bytes) { return tab.add(bytes); });
    const size_t blob_off = tab.add(blob_bytes);

    int rc;
    if ((rc = tab.take())) return rc;
    planner.pack(tab.at<unsigned char>(0));          // (before the records are copied: packing completes the plans)
    if (blob_bytes) memcpy(tab.at<unsigned char>(blob_off), blob_host, blob_bytes);
    if ((rc = vkx_scratch_reserve(ctx, &ctx->layer_tables, std::max(tab.bytes, (size_t)256 << 10)))) return rc;
    unsigned char *base = (unsigned char *)ctx->layer_tables.ptr;
    for (int i = 0; i < n_layers; i++)
        if (layers_host[i].kind != VKX_LAYER_FRAME && layers_host[i].src_off >= 0) recs[i].src = base + blob_off + layers_host[i].src_off;
    memcpy(tab.at<LayerRec>(recs_off), recs.data(), sizeof(LayerRec) * (size_t)n_layers);
    const auto put_grid = [&](size_t off, const std::vector<int> &which, const std::vector<int> &starts) {
        if (!which.empty()) memcpy(tab.at<int>(off), which.data(), sizeof(int) * which.size());
        memcpy(tab.at<int>(off) + which.size(), starts.data(), sizeof(int) * starts.size());
    };
    put_grid(sym_off, sym_which, sym_starts);
    put_grid(pln_off, pln_which, pln_starts);
    memset(tab.at<unsigned>(max_off), 0, sizeof(unsigned) * (size_t)n_layers);
    if ((rc = tab.copy_to(ctx->layer_tables.ptr))) return rc;
    const LayerRec *d_recs = (const LayerRec *)(base + recs_off);
    unsigned *rec_max = (unsigned *)(base + max_off);
    if (!sym_which.empty()) {
        const int *which = (const int *)(base + sym_off);
        VKX_TIMED(ctx, "k_layer_symbols");
        k_layer_symbols<<<(unsigned)sym_starts.back(), 256, 0, ctx->stream>>>(d_recs, which, which + sym_which.size(), (int)sym_which.size(), base, rec_max);
        VKX_LAUNCH_CHECK();
    }
    if (!pln_which.empty()) {
        const int *which = (const int *)(base + pln_off);
        VKX_TIMED(ctx, "k_layer_planes");
        k_layer_planes<<<(unsigned)pln_starts.back(), 256, 0, ctx->stream>>>(d_recs, which, which + pln_which.size(), (int)pln_which.size(), base, rec_max);
        VKX_LAUNCH_CHECK();
    }
    return VKX_OK;
}
