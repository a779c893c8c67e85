// The text-region labels of PageTextRegionLabelStep on gfx950 (reference: pipeline/text_detection/page_text_region_label.py).
//
// Two entry points, one launch each:
//   k_region_label_deviate  the deviate candidates of the char regression labels (:498-575).  One workgroup takes a run of
//                           chars: one lane per char computes the homography bbox corners -> the polygon's self-relative
//                           integer points (vkc::quad_internals and vkc::perspective_transform, shared with char_mask.hip
//                           and char_heatmap.hip) into LDS, then one lane per candidate maps its drawn point as
//                           affine_points does (vkc::affine_point), adds the box origin,
//                           reports the page status and the rounded point, and compares its squared distance to every
//                           centre (staged through LDS tiles, exact 64-bit integers) with the distance to its own char's
//                           centre: keep (own strictly nearest), drop (another strictly nearer) or tie (left to the host).
//   k_region_label_planes   the char bounding-box mask (the union of the chars' floor / ceil boxes) and the inactive region:
//                           one workgroup per 32 x 32 page tile; the host bins the boxes into tiles (vkb::TileBins; a tile a
//                           box covers whole is only flagged and lists nothing), a lane writes 4 pixels: the mask, and 0 into the char mask and the height map
//                           where the active mask is 0.
// Every value is written with plain vector stores; no atomics.
#include "vkx_cell.h"
#include "vkx_internal.h"
#include "vkx_tile_bins.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kDevBlock = 128;        // lanes of a deviate workgroup (two waves)
constexpr int kCentreTile = 256;      // centres staged per LDS tile
constexpr int kMaxSide = 32768;       // page sides: rounded points and their squared distances stay exact
constexpr int kMaxCandidates = 4096;  // candidates per char
constexpr long long kMaxCentre = 1LL << 30;
constexpr int kTile = 32;             // planes: 32 x 32 pixels per workgroup, 4 per lane
constexpr long long kMaxEntries = 1ll << 28;     // (box, tile) pairs of one call, as quad_interp.hip has it

__global__ void __launch_bounds__(kDevBlock) k_region_label_deviate(const double *__restrict__ quads, const int *__restrict__ boxes,
                                                                   const int2 *__restrict__ centres, int n_centres, int n_chars,
                                                                   const int2 *__restrict__ draws, int m, int chars_per_block,
                                                                   int h, int w, vkx_region_label_deviate_out *__restrict__ out)
{
    __shared__ double sH[kDevBlock][9];
    __shared__ int2 sC[kCentreTile];
    const int c0 = blockIdx.x * chars_per_block;
    const int nc = min(chars_per_block, n_chars - c0);
    if ((int)threadIdx.x < nc) {
        const int g = c0 + threadIdx.x;
        const double *q = quads + (size_t)g * 8;
        float rel[8];
        vkc::quad_internals(q, rel);
        const int *b = boxes + (size_t)g * 4;
        const float ex = (float)(b[3] - 1), ey = (float)(b[2] - 1);
        const float src[8] = {0.f, 0.f, ex, 0.f, ex, ey, 0.f, ey};
        double H[9];
        vkc::perspective_transform(src, rel, H);
        for (int k = 0; k < 9; k++) sH[threadIdx.x][k] = H[k];
    }
    __syncthreads();

    const int total = nc * m;
    for (int base = 0; base < total; base += kDevBlock) {       // uniform over the workgroup: every lane reaches the barriers
        const int k = base + threadIdx.x;
        const bool active = k < total;
        int g = 0, status = 0, iy = 0, ix = 0;
        double ay = 0.0, ax = 0.0;
        long long d_own = 0, d_other = LLONG_MAX;
        if (active) {
            const int lc = k / m, j = k - lc * m;
            g = c0 + lc;
            const double *H = sH[lc];
            const int2 d = draws[(size_t)g * m + j];           // (x, y) in the shifted bounding box
            double px, py;
            vkc::affine_point(H, (double)d.x, (double)d.y, m == 1, px, py);
            const int *b = boxes + (size_t)g * 4;
            if (!isfinite(px) || !isfinite(py)) {
                status = 3;                                     // round() of the point raises
            } else {
                if (j == m - 1 && m > 2) {
                    // PointTuple.from_np_array drops a last point equal (as integers) to the first one
                    const int2 d0 = draws[(size_t)g * m];
                    double px0, py0;
                    vkc::affine_point(H, (double)d0.x, (double)d0.y, false, px0, py0);
                    if (isfinite(px0) && isfinite(py0) && rint(px0) == rint(px) && rint(py0) == rint(py)) status = 1;
                }
                ay = (double)b[0] + py;
                ax = (double)b[1] + px;
                if (status == 0 && !(0.0 <= ay && ay < (double)h && 0.0 <= ax && ax < (double)w)) status = 2;
                if (status == 0) {
                    iy = (int)rint(ay);
                    ix = (int)rint(ax);
                    const int2 c = centres[g];
                    const long long dy = (long long)iy - c.y, dx = (long long)ix - c.x;
                    d_own = dx * dx + dy * dy;
                }
            }
        }
        for (int t0 = 0; t0 < n_centres; t0 += kCentreTile) {
            const int nt = min(kCentreTile, n_centres - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < nt; i += kDevBlock) sC[i] = centres[t0 + i];
            __syncthreads();
            if (active && status == 0) {
                for (int i = 0; i < nt; i++) {
                    if (t0 + i == g) continue;
                    const long long dy = (long long)iy - sC[i].y, dx = (long long)ix - sC[i].x;
                    d_other = min(d_other, dx * dx + dy * dy);
                }
            }
        }
        if (active) {
            vkx_region_label_deviate_out o;
            o.y = ay;
            o.x = ax;
            o.iy = iy;
            o.ix = ix;
            o.status = status;
            o.cls = status ? 0 : (d_own < d_other ? 0 : (d_other < d_own ? 1 : 2));
            out[(size_t)c0 * m + k] = o;
        }
    }
}

__global__ void __launch_bounds__(256) k_region_label_planes(const int4 *__restrict__ boxes, const int *__restrict__ tile_start,
                                                             const int *__restrict__ entries, const uint8_t *__restrict__ full,
                                                             int tiles_x, int h, int w, const uint8_t *__restrict__ active,
                                                             uint8_t *__restrict__ char_mask, float *__restrict__ height,
                                                             uint8_t *__restrict__ box_mask)
{
    const int t = blockIdx.x;
    int x, y0;                                                 // 256 lanes: the first 8 rows of the tile
    if (!vkd::tile_pixel<kTile, kTile>(tiles_x, h, w, x, y0)) return;
    const bool whole = full[t] != 0;
    const int e0 = tile_start[t], e1 = tile_start[t + 1];
    for (int r = 0; r < kTile; r += 8) {
        const int y = y0 + r;
        if (y >= h) break;
        bool covered = whole;
        for (int e = e0; e < e1 && !covered; e++) {
            const int4 b = boxes[entries[e]];                  // (up, down, left, right), inside the page
            covered = b.x <= y && y <= b.y && b.z <= x && x <= b.w;
        }
        const size_t i = (size_t)y * w + x;
        box_mask[i] = covered ? 1 : 0;
        if (active[i] == 0) {
            char_mask[i] = 0;
            height[i] = 0.f;
        }
    }
}

}  // namespace

VKX_EXPORT int vkx_region_label_deviate_dev(vkx_ctx *ctx, const double *quads_host, const int32_t *centres_host, int n_centres,
                                            int n_chars, const int32_t *draws_host, int m, int h, int w,
                                            vkx_region_label_deviate_out *out)
{
    VKX_REQUIRE(ctx && quads_host && centres_host && draws_host && out, "NULL argument");
    VKX_REQUIRE(n_centres >= 1 && n_centres < (1 << 24), "1 .. 2^24 - 1 centres");
    VKX_REQUIRE(n_chars >= 1 && n_chars <= n_centres, "1 .. n_centres chars");
    VKX_REQUIRE(m >= 1 && m <= kMaxCandidates, "1 .. 4096 candidates per char");
    VKX_REQUIRE((long long)n_chars * m < (1LL << 31), "too many candidates");
    VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "page sides 1 .. 32768");
    for (int g = 0; g < n_centres; g++) {
        const long long cx = centres_host[2 * g], cy = centres_host[2 * g + 1];
        VKX_REQUIRE(cx > -kMaxCentre && cx < kMaxCentre && cy > -kMaxCentre && cy < kMaxCentre, "centre outside +-2^30");
    }
    // the boxes (up, left, bh, bw) from the rounded points, as Polygon.bounding_box; every draw inside [1, b - 2]
    std::vector<int> boxes((size_t)4 * n_chars);
    for (int g = 0; g < n_chars; g++) {
        const double *q = quads_host + (size_t)g * 8;
        double box[4];
        VKX_REQUIRE(vkx_quad_box(q, box), "non-finite char point");
        for (int k = 0; k < 8; k++) VKX_REQUIRE(std::fabs(q[k]) < kMaxCentre, "char point outside +-2^30");
        int *b = boxes.data() + (size_t)4 * g;
        for (int k = 0; k < 4; k++) b[k] = (int)box[k];
        VKX_REQUIRE(b[2] >= 3 && b[3] >= 3, "a char box narrower than 3 pixels has no candidates");
        for (int j = 0; j < m; j++) {
            const int32_t *d = draws_host + ((size_t)g * m + j) * 2;
            VKX_REQUIRE(d[0] >= 1 && d[0] <= b[3] - 2 && d[1] >= 1 && d[1] <= b[2] - 2, "a draw outside [1, box - 2]");
        }
    }
    vkx_tables tab(ctx);
    const size_t quad_off = tab.add((size_t)n_chars * 64), box_off = tab.add((size_t)n_chars * 16);
    const size_t centre_off = tab.add((size_t)n_centres * 8), draw_off = tab.add((size_t)n_chars * m * 8);
    int rc = tab.take();
    if (rc) return rc;
    memcpy(tab.at<double>(quad_off), quads_host, (size_t)n_chars * 64);
    memcpy(tab.at<int>(box_off), boxes.data(), (size_t)n_chars * 16);
    memcpy(tab.at<int32_t>(centre_off), centres_host, (size_t)n_centres * 8);
    memcpy(tab.at<int32_t>(draw_off), draws_host, (size_t)n_chars * m * 8);
    if ((rc = tab.copy_to(&ctx->rl_deviate, (size_t)64 << 10))) return rc;
    char *base = (char *)ctx->rl_deviate.ptr;
    const int chars_per_block = std::max(1, kDevBlock / m);
    {
        VKX_TIMED(ctx, "k_region_label_deviate");
        k_region_label_deviate<<<vkx_blocks(n_chars, chars_per_block), kDevBlock, 0, ctx->stream>>>(
            (const double *)(base + quad_off), (const int *)(base + box_off), (const int2 *)(base + centre_off), n_centres,
            n_chars, (const int2 *)(base + draw_off), m, chars_per_block, h, w, out);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_region_label_planes_dev(vkx_ctx *ctx, const int32_t *boxes_host, int n_boxes, int h, int w,
                                           const uint8_t *active_mask, uint8_t *char_mask, float *char_height,
                                           uint8_t *box_mask)
{
    VKX_REQUIRE(ctx && (boxes_host || n_boxes == 0) && active_mask && char_mask && char_height && box_mask, "NULL argument");
    VKX_REQUIRE(n_boxes >= 0 && n_boxes < (1 << 24), "0 .. 2^24 - 1 boxes");
    VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "page sides 1 .. 32768");
    const size_t page = (size_t)h * w;
    const vkx_plane_bytes planes[4] = {{active_mask, page}, {char_mask, page}, {char_height, page * 4}, {box_mask, page}};
    VKX_REQUIRE(vkx_planes_disjoint(planes, 4), "planes overlap");
    for (int k = 0; k < n_boxes; k++) {
        const int32_t *b = boxes_host + (size_t)4 * k;
        VKX_REQUIRE(0 <= b[0] && b[0] <= b[1] && b[1] < h && 0 <= b[2] && b[2] <= b[3] && b[3] < w, "a box outside the page");
    }
    // bin the boxes into 32 x 32 tiles: a tile a box covers whole is flagged, the others list the box
    vkb::TileBins<kTile, kTile> bins(h, w);
    const int tiles = (int)bins.n_tiles();
    std::vector<uint8_t> full((size_t)tiles, 0);
    // the tiles with every row inside lo .. hi: a clipped last tile ends where the page does
    auto whole = [](int lo, int hi, int len, int &t0, int &t1) {
        t0 = (lo + kTile - 1) / kTile;
        t1 = hi == len - 1 ? (len - 1) / kTile : (hi + 1) / kTile - 1;
    };
    for (int k = 0; k < n_boxes; k++) {
        const int32_t *b = boxes_host + (size_t)4 * k;
        int ty0, ty1, tx0, tx1;
        whole(b[0], b[1], h, ty0, ty1);
        whole(b[2], b[3], w, tx0, tx1);
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) full[(size_t)ty * bins.tiles_x + tx] = 1;
    }
    auto span_of = [&](int k) {
        const int32_t *b = boxes_host + (size_t)4 * k;
        return bins.rect(b[0], b[1], b[2], b[3]);
    };
    auto listed = [&](size_t t, int) { return !full[t]; };
    VKX_REQUIRE(bins.count(n_boxes, kMaxEntries, span_of, listed), "too many (box, tile) pairs");

    vkx_tables tab(ctx);
    const size_t box_off = tab.add((size_t)n_boxes * 16), start_off = tab.add(((size_t)tiles + 1) * 4);
    const size_t entry_off = tab.add(std::max<size_t>(bins.pairs(), 1) * 4), full_off = tab.add((size_t)tiles);
    int rc = tab.take();
    if (rc) return rc;
    if (n_boxes) memcpy(tab.at<int32_t>(box_off), boxes_host, (size_t)n_boxes * 16);
    memcpy(tab.at<int>(start_off), bins.start.data(), ((size_t)tiles + 1) * 4);
    *tab.at<int>(entry_off) = 0;                               // (a call without pairs stages one entry)
    bins.fill(n_boxes, tab.at<int>(entry_off), span_of, listed);
    memcpy(tab.at<uint8_t>(full_off), full.data(), (size_t)tiles);
    if ((rc = tab.copy_to(&ctx->rl_planes, (size_t)64 << 10))) return rc;
    char *base = (char *)ctx->rl_planes.ptr;
    {
        VKX_TIMED(ctx, "k_region_label_planes");
        k_region_label_planes<<<(unsigned)tiles, 256, 0, ctx->stream>>>(
            (const int4 *)(base + box_off), (const int *)(base + start_off), (const int *)(base + entry_off),
            (const uint8_t *)(base + full_off), bins.tiles_x, h, w, active_mask, char_mask, char_height, box_mask);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
