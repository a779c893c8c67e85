// The default char-heatmap engine on gfx950 (reference: engine/char_heatmap/default.py:93-180).
//
// Per char the reference warps a Gaussian template into the char's quad (getPerspectiveTransform + warpPerspective into the
// char's bounding box), keeps the max and the min of the warped values over the char's fillPoly raster, counts the chars
// that cover every pixel (Mask.from_polygons INTERSECT), and mixes the page planes with numpy.  Here one call takes every
// char of one page and writes fresh planes in three launches and no synchronisation:
//   k_char_heatmap_setup    one lane per char: the homography (vkc::quad_internals and vkc::perspective_transform, shared with
//                           char_mask.hip), the warpPerspective coordinate map of the char's box and the 4 edges of its
//                           fillPoly test;
//   k_char_heatmap_raster   one workgroup per 32 x 8 tile of a char's box (the host computes the boxes itself, vkx_quad_box, and
//                           lays the tiles out from them, vkb::box_tile_starts; vkd::box_tile_pixel): a lane decides the fillPoly membership of its pixel in closed form (the
//                           LINE_8 outline by vkc::bres_minor, or inside an even-odd span of the 16.16 crossings), samples
//                           the template (vkd::CoordPerspective + vkd::sample_f32) and takes atomicMax / atomicMin of the
//                           float bits into two page-sized int planes and atomicAdd into a count plane;
//   k_char_heatmap_resolve  every page pixel: the numpy tail of the reference (preserving / neutralized masks, the clipped
//                           delta, the weighted score) and the three scratch words back to their initial values.
// Every value is >= +0.0, so integer order is float order and the result does not depend on the order of arrival; each
// (char, pixel) pair is visited once, so the count needs no deduplication.
#include "vkx_cell.h"
#include "vkx_internal.h"
#include "vkx_poly_raster.h"
#include "vkx_tile_bins.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kTileW = 32, kTileH = 8;     // one lane per pixel; a wave covers two 128-B row segments of each plane
constexpr int kMaxRadius = 1024;
constexpr int kMaxSide = 1 << 24;          // page sides below 2^24: the float32 integer points of the reference are exact
constexpr int kOneBits = 0x3f800000;       // 1.0f: the initial min

struct CharHeat {             // what the setup pass leaves for the raster
    vkd::CoordPerspective coord;
    vkp::Edge e[4];           // of the char's integer quad, vertex (i + 3) & 3 -> vertex i (vkp::quad_covers)
    int up, left, bh, bw;     // the bounding box in page coordinates
};

__global__ void __launch_bounds__(256) k_char_heatmap_setup(const double *__restrict__ quads, const int *__restrict__ boxes,
                                                            int n, int r, CharHeat *__restrict__ heat)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const double *q = quads + (size_t)g * 8;
    float rel[8];                        // Polygon.internals: relative to the box's up / left
    vkc::quad_internals(q, rel);
    const float s = (float)(2 * r);
    const float tmpl_pts[8] = {0.f, 0.f, s, 0.f, s, s, 0.f, s};
    double H[9];
    vkc::perspective_transform(tmpl_pts, rel, H);
    CharHeat C;
    const int *b = boxes + (size_t)g * 4;
    C.up = b[0]; C.left = b[1]; C.bh = b[2]; C.bw = b[3];
    C.coord = vkd::make_perspective(H, C.bh, C.bw);        // warpPerspective(template, H, (bbox.width, bbox.height))
    int vx[4], vy[4];
    for (int k = 0; k < 4; k++) { vx[k] = (int)rel[2 * k]; vy[k] = (int)rel[2 * k + 1]; }
    for (int i = 0; i < 4; i++) C.e[i] = vkp::make_edge(vx[(i + 3) & 3], vy[(i + 3) & 3], vx[i], vy[i]);
    heat[g] = C;
}

// one workgroup per 32 x 8 tile of a char box; tile_start[g] .. tile_start[g + 1] are char g's tiles
__global__ void __launch_bounds__(256) k_char_heatmap_raster(const CharHeat *__restrict__ heat, const int *__restrict__ tile_start,
                                                             int n, const float *__restrict__ tmpl, int E, int w,
                                                             int *__restrict__ max_bits, int *__restrict__ min_bits,
                                                             int *__restrict__ count)
{
    int rx, ry;
    const int lo = vkd::box_tile_pixel<kTileW, kTileH>(n, tile_start, [&](int g) { return heat[g].bw; }, rx, ry);     // the char of the tile
    const CharHeat &C = heat[lo];
    if (ry >= C.bh || rx >= C.bw) return;
    if (!vkp::quad_covers(C.e, rx, ry)) return;
    int X, Y;
    C.coord(rx, ry, X, Y);
    const float v = vkd::sample_f32(tmpl, E, E, E, X, Y);
    const size_t i = (size_t)(C.up + ry) * w + (C.left + rx);     // inside the page: the host checked every box
    const int bits = __float_as_int(v);
    atomicMax(max_bits + i, bits);
    atomicMin(min_bits + i, bits);
    atomicAdd(count + i, 1);
}

struct Planes {
    float *score;
    float *max, *min, *delta, *nscore;        // debug planes (all NULL or all set)
    uint8_t *overlapped, *neutralized;
};

__global__ void __launch_bounds__(256) k_char_heatmap_resolve(int *__restrict__ max_bits, int *__restrict__ min_bits,
                                                              int *__restrict__ count, size_t page, float preserving,
                                                              float weight_max, float weight_neutralized, Planes P)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= page) return;
    const int c = count[i];
    const float mx = c ? __int_as_float(max_bits[i]) : 0.f;
    const float mn = c ? __int_as_float(min_bits[i]) : 1.f;
    if (c) { max_bits[i] = 0; min_bits[i] = kOneBits; count[i] = 0; }
    const bool overlapped = c >= 2;                        // Mask.from_polygons(INTERSECT): active count > 1
    const bool neutralized = overlapped && !(mx >= preserving);
    const float delta = fminf(fmaxf(mx - mn, 0.f), 1.f);   // np.clip(max - min, 0.0, 1.0)
    const float ns = neutralized ? delta : mx;
    const float a = weight_max * mx, b = weight_neutralized * ns;
    P.score[i] = a + b;
    if (P.max) {
        P.max[i] = mx;
        P.min[i] = mn;
        P.overlapped[i] = overlapped;
        P.delta[i] = delta;
        P.neutralized[i] = neutralized;
        P.nscore[i] = ns;
    }
}

// The output planes of one call, in the order of the checks and the copies of the host form.
struct OutPlane { void *p; size_t elem; };

int collect_outputs(float *score, const vkx_char_heatmap_debug *debug, OutPlane out[7], int *n_out)
{
    VKX_REQUIRE(score, "NULL argument");
    out[0] = {score, 4};
    *n_out = 1;
    if (debug) {
        VKX_REQUIRE(debug->score_map_max && debug->score_map_min && debug->char_overlapped_mask &&
                        debug->char_neutralized_score_map && debug->neutralized_mask && debug->neutralized_score_map,
                    "a debug record needs all six planes");
        out[1] = {debug->score_map_max, 4};
        out[2] = {debug->score_map_min, 4};
        out[3] = {debug->char_overlapped_mask, 1};
        out[4] = {debug->char_neutralized_score_map, 4};
        out[5] = {debug->neutralized_mask, 1};
        out[6] = {debug->neutralized_score_map, 4};
        *n_out = 7;
    }
    return VKX_OK;
}

// Argument checks shared by both forms; boxes (up, left, bh, bw) of every char on success.
int check_call(const vkx_char_heatmap_config *config, const double *quads, int n, int h, int w, float *score,
               const vkx_char_heatmap_debug *debug, std::vector<int> *boxes)
{
    VKX_REQUIRE(config && (quads || n == 0), "NULL argument");
    VKX_REQUIRE(config->radius >= 1 && config->radius <= kMaxRadius, "radius 1 .. 1024");
    VKX_REQUIRE(config->template_host, "NULL template");
    VKX_REQUIRE(n >= 0 && n < (1 << 24), "0 .. 2^24 - 1 chars");
    VKX_REQUIRE(h >= 1 && w >= 1 && h < kMaxSide && w < kMaxSide && (long long)h * w < (1LL << 31), "bad page shape");
    OutPlane out[7];
    int n_out = 0;
    int rc = collect_outputs(score, debug, out, &n_out);
    if (rc) return rc;
    const size_t page = (size_t)h * w;
    vkx_plane_bytes planes[7];
    for (int k = 0; k < n_out; k++) planes[k] = {out[k].p, page * out[k].elem};
    VKX_REQUIRE(vkx_planes_disjoint(planes, n_out), "output planes overlap");
    boxes->assign((size_t)4 * n, 0);
    for (int g = 0; g < n; g++) {
        double box[4];
        VKX_REQUIRE(vkx_quad_box(quads + (size_t)g * 8, box), "non-finite char point");
        VKX_REQUIRE(box[0] >= 0 && box[0] + box[2] <= h && box[1] >= 0 && box[1] + box[3] <= w, "a char box outside the page");
        for (int k = 0; k < 4; k++) (*boxes)[(size_t)4 * g + k] = (int)box[k];
    }
    return VKX_OK;
}

}  // namespace

VKX_EXPORT int vkx_char_heatmap_fresh_dev(vkx_ctx *ctx, const vkx_char_heatmap_config *config, const double *quads_host, int n_chars,
                                          int h, int w, float *score, const vkx_char_heatmap_debug *debug)
{
    VKX_REQUIRE(ctx, "NULL argument");
    std::vector<int> boxes;
    int rc = check_call(config, quads_host, n_chars, h, w, score, debug, &boxes);
    if (rc) return rc;
    const int n = n_chars, r = config->radius, E = 2 * r + 1;

    // the tile layout, from the boxes
    std::vector<int> tile_start;
    VKX_REQUIRE((vkb::box_tile_starts<kTileW, kTileH>(n, [&](int g, long long &bh, long long &bw) {
                    bh = boxes[(size_t)4 * g + 2]; bw = boxes[(size_t)4 * g + 3]; }, tile_start)),
                "too many tiles");
    const int tiles = tile_start[n];

    // one staged block: template, quads, boxes, tile starts
    vkx_tables tab(ctx);
    const size_t tmpl_off = tab.add((size_t)E * E * 4), quad_off = tab.add((size_t)n * 64), box_off = tab.add((size_t)n * 16);
    const size_t tile_off = tab.add(sizeof(int) * tile_start.size());
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<float>(tmpl_off), config->template_host, (size_t)E * E * 4);
    if (n) {
        memcpy(tab.at<double>(quad_off), quads_host, (size_t)n * 64);
        memcpy(tab.at<int>(box_off), boxes.data(), (size_t)n * 16);
    }
    memcpy(tab.at<int>(tile_off), tile_start.data(), sizeof(int) * tile_start.size());
    if ((rc = tab.copy_to(&ctx->heat_table, (size_t)64 << 10))) return rc;
    char *base = (char *)ctx->heat_table.ptr;
    const float *tmpl_dev = (const float *)(base + tmpl_off);
    const double *quads_dev = (const double *)(base + quad_off);
    const int *boxes_dev = (const int *)(base + box_off);
    const int *tiles_dev = (const int *)(base + tile_off);
    if ((rc = vkx_scratch_reserve(ctx, &ctx->heat_geo, std::max(sizeof(CharHeat) * (size_t)n, (size_t)64 << 10)))) return rc;
    CharHeat *heat = (CharHeat *)ctx->heat_geo.ptr;

    // the max / min / count planes: max 0, min 1.0f, count 0 between calls for the page size they were last set up for
    const size_t page = (size_t)h * w;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->heat_planes, 3 * sizeof(int) * page))) return rc;
    int *max_bits = (int *)ctx->heat_planes.ptr, *min_bits = max_bits + page, *count = min_bits + page;
    {
        vkx_device_guard guard(ctx);
        if (ctx->heat_clean_page != page) {
            VKX_HIP(hipMemsetAsync(max_bits, 0, sizeof(int) * page, ctx->stream));
            VKX_HIP(hipMemsetD32Async((hipDeviceptr_t)min_bits, kOneBits, page, ctx->stream));
            VKX_HIP(hipMemsetAsync(count, 0, sizeof(int) * page, ctx->stream));
        }
    }
    ctx->heat_clean_page = 0;

    if (n) {
        {
            VKX_TIMED(ctx, "k_char_heatmap_setup");
            k_char_heatmap_setup<<<vkx_blocks(n, 64), 64, 0, ctx->stream>>>(quads_dev, boxes_dev, n, r, heat);
        }
        VKX_LAUNCH_CHECK();
        {
            VKX_TIMED(ctx, "k_char_heatmap_raster");
            k_char_heatmap_raster<<<(unsigned)tiles, 256, 0, ctx->stream>>>(heat, tiles_dev, n, tmpl_dev, E, w, max_bits,
                                                                             min_bits, count);
        }
        VKX_LAUNCH_CHECK();
    }
    Planes P;
    P.score = score;
    P.max = debug ? debug->score_map_max : nullptr;
    P.min = debug ? debug->score_map_min : nullptr;
    P.overlapped = debug ? debug->char_overlapped_mask : nullptr;
    P.delta = debug ? debug->char_neutralized_score_map : nullptr;
    P.neutralized = debug ? debug->neutralized_mask : nullptr;
    P.nscore = debug ? debug->neutralized_score_map : nullptr;
    {
        VKX_TIMED(ctx, "k_char_heatmap_resolve");
        k_char_heatmap_resolve<<<vkx_blocks(page, 256), 256, 0, ctx->stream>>>(
            max_bits, min_bits, count, page, config->preserving_score_min, config->weight_max, config->weight_neutralized, P);
    }
    VKX_LAUNCH_CHECK();
    ctx->heat_clean_page = page;
    return VKX_OK;
}

// The host form: planes in host memory, staged through device scratch; returns after the copies back.
VKX_EXPORT int vkx_char_heatmap_fresh(vkx_ctx *ctx, const vkx_char_heatmap_config *config, const double *quads_host, int n_chars,
                                      int h, int w, float *score, const vkx_char_heatmap_debug *debug)
{
    VKX_REQUIRE(ctx, "NULL argument");
    std::vector<int> boxes;
    int rc = check_call(config, quads_host, n_chars, h, w, score, debug, &boxes);
    if (rc) return rc;
    OutPlane out[7];
    int n_out = 0;
    if ((rc = collect_outputs(score, debug, out, &n_out))) return rc;
    const size_t page = (size_t)h * w;
    size_t at[7], bytes = 0;
    for (int k = 0; k < n_out; k++) {
        at[k] = bytes;
        bytes += vkx_align256(page * out[k].elem);
    }
    if ((rc = vkx_scratch_reserve(ctx, &ctx->heat_host, bytes))) return rc;
    char *base = (char *)ctx->heat_host.ptr;
    vkx_char_heatmap_debug dev_debug;
    if (debug) {
        dev_debug.score_map_max = (float *)(base + at[1]);
        dev_debug.score_map_min = (float *)(base + at[2]);
        dev_debug.char_overlapped_mask = (uint8_t *)(base + at[3]);
        dev_debug.char_neutralized_score_map = (float *)(base + at[4]);
        dev_debug.neutralized_mask = (uint8_t *)(base + at[5]);
        dev_debug.neutralized_score_map = (float *)(base + at[6]);
    }
    if ((rc = vkx_char_heatmap_fresh_dev(ctx, config, quads_host, n_chars, h, w, (float *)base, debug ? &dev_debug : nullptr)))
        return rc;
    vkx_device_guard guard(ctx);
    for (int k = 0; k < n_out; k++)
        VKX_HIP(hipMemcpyAsync(out[k].p, base + at[k], page * out[k].elem, hipMemcpyDeviceToHost, ctx->stream));
    VKX_HIP(hipStreamSynchronize(ctx->stream));
    return VKX_OK;
}
