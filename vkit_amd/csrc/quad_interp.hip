// Text-line labels on gfx950 (reference: element/score_map.py:139-283 ScoreMap.from_quad_interpolation, :562-588
// fill_by_quad_interpolation; pipeline/text_detection/page_text_line_label.py:156-306 the masks and the boundary score map).
//
// from_quad_interpolation inverts the bilinear map of a quad per pixel of its bounding box: a quadratic in v whose root is chosen
// by a vote over the whole quad, then u from v.  The vote is why a batch of quads takes two launches:
//   k_quad_vote   one wave per 64 bounding-box pixels of a quad on the quadratic branch: the lanes under the quad's raster ballot
//                 "my positive / negative root lies in [0, 1]", lane 0 adds the two popcounts to the quad's int32 pair.  Integer
//                 sums: the result does not depend on the order of the atomics.
//   k_quad_fill   one workgroup per 32 x 8 tile of dst; a pixel keeps dst in a register, walks the quads binned to its tile IN
//                 LIST ORDER (the host bins them, vkb::TileBins; a tile's list has any length, it is read entry by entry, not in chunks),
//                 applies the fill rule of each, then the zeroing plane, and stores once.
//   k_quad_uv     the raw (u, v) planes of one quad (an arbitrary func_np_uv_to_mat runs on the host).
//   k_box_masks   the three masks of PageTextLineLabelStep over the same tile bins: one launch.
// The raster of a quad is vkp::quad_covers on its integer vertices (vkx_poly_raster.h).  The arithmetic is the reference's as
// numpy 2 evaluates it (include/vkx.h states it); float32 quotients and roots are formed in float64 and rounded once more, which
// is the correctly rounded float32 result (53 >= 2 * 24 + 2) whatever the compiler's float32 division is.  The library is built
// with -ffp-contract=off: no product below is fused into a sum.  Vector atomics and plain vector stores only.
#include "vkx_internal.h"
#include "vkx_poly_raster.h"
#include "vkx_tile_bins.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kMaxSide = 32768;
constexpr int kMaxQuads = (1 << 24) - 1;
constexpr int kTileW = 32, kTileH = 8;
constexpr long long kMaxEntries = 1ll << 28;     // (record, tile) pairs of one call
typedef vkb::TileBins<kTileW, kTileH> Bins;      // every tile lists its quads, or boxes, in ascending index

struct QuadRec {
    vkp::Edge e[4];                  // of the self-relative integer quad, vertex (i + 3) & 3 -> vertex i
    float x0, y0;                    // vertex 0
    float b1x, b1y, b2x, b2y, b3x, b3y;
    float b1xb2;                     // b1 x b2
    float four_a, i2a;               // float32(4 * a), float32(0.5 / a): the Python floats as numpy casts them to the arrays' type
    int quadratic, comp;
    int up, left, bh, bw;            // the bounding box in dst
    int pad;
};

struct VoteRec { int quad, wave_base; };     // a quad on the quadratic branch and the prefix of its 64-pixel groups

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }

__device__ __forceinline__ void coeffs(const QuadRec &r, int ix, int iy, double &qx, double &qy, float &b, float &c)
{
    qx = (double)ix - (double)r.x0;
    qy = (double)iy - (double)r.y0;
    const double b3q = (double)r.b3x * qy - (double)r.b3y * qx;
    b = (float)(b3q - (double)r.b1xb2);
    c = (float)((double)r.b1x * qy - (double)r.b1y * qx);
}

__device__ __forceinline__ void roots(const QuadRec &r, float b, float c, float &v_pos, float &v_neg)
{
    const float bb = b * b, ac = r.four_a * c;
    const float discrim = sqrt_rn(bb - ac);
    v_pos = (-b + discrim) * r.i2a;
    v_neg = (-b - discrim) * r.i2a;
}

__device__ __forceinline__ bool in_unit(float v) { return 0.0f <= v && v <= 1.0f; }
// np.clip: a NaN stays, and so does -0.0
__device__ __forceinline__ float clip_unit(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// (u, v) of a pixel under the quad's raster
__device__ __forceinline__ void solve(const QuadRec &r, int ix, int iy, bool use_neg, bool want_u, float &u, float &v)
{
    double qx, qy;
    float b, c;
    coeffs(r, ix, iy, qx, qy, b, c);
    if (r.quadratic) {
        float v_pos, v_neg;
        roots(r, b, c, v_pos, v_neg);
        v = use_neg ? v_neg : v_pos;
    } else {
        v = div_rn(-c, b);
    }
    v = clip_unit(v);
    u = 0.0f;
    if (!want_u) return;
    const float px = r.b3x * v, py = r.b3y * v;
    const float dx = r.b1x + px, dy = r.b1y + py;
    if (fabsf(dx) > fabsf(dy) && dx != 0.0f) {
        const float s = r.b2x * v;
        u = (float)((qx - (double)s) / (double)dx);
    } else if (dy != 0.0f) {         // (true for a NaN, as in numpy)
        const float s = r.b2y * v;
        u = (float)((qy - (double)s) / (double)dy);
    }
    u = clip_unit(u);
}

// grid: 4 waves a workgroup over the 64-pixel groups of the quads of `list`
__global__ void __launch_bounds__(256) k_quad_vote(const QuadRec *__restrict__ recs, const VoteRec *__restrict__ list, int n_list,
                                                   int total_waves, int *__restrict__ votes)
{
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wv >= total_waves) return;                      // (the whole wave)
    const VoteRec vr = list[vkd::last_at_most(n_list, wv, [&](int i) { return list[i].wave_base; })];
    const QuadRec &r = recs[vr.quad];
    const int idx = (wv - vr.wave_base) * 64 + lane;
    bool pos = false, neg = false;
    if (idx < r.bh * r.bw) {
        const int iy = idx / r.bw, ix = idx - iy * r.bw;
        if (vkp::quad_covers(r.e, ix, iy)) {
            double qx, qy;
            float b, c, v_pos, v_neg;
            coeffs(r, ix, iy, qx, qy, b, c);
            roots(r, b, c, v_pos, v_neg);
            pos = in_unit(v_pos);
            neg = in_unit(v_neg);
        }
    }
    const int n_pos = __popcll(__ballot(pos)), n_neg = __popcll(__ballot(neg));
    if (lane == 0) {
        if (n_pos) atomicAdd(&votes[2 * vr.quad], n_pos);
        if (n_neg) atomicAdd(&votes[2 * vr.quad + 1], n_neg);
    }
}

// grid: the tiles of dst
__global__ void __launch_bounds__(256) k_quad_fill(const QuadRec *__restrict__ recs, const int *__restrict__ tile_start,
                                                   const int *__restrict__ tile_list, const int *__restrict__ votes, int mode, int fresh,
                                                   int h, int w, int tiles_x, float *__restrict__ dst, const uint8_t *__restrict__ zero_where)
{
    int x, y;
    if (!vkd::tile_pixel<kTileW, kTileH>(tiles_x, h, w, x, y)) return;
    const int begin = tile_start[blockIdx.x], end = tile_start[blockIdx.x + 1];
    const size_t p = (size_t)y * w + x;
    if (zero_where && zero_where[p] == 0) {             // whatever the quads leave here is zeroed after them
        dst[p] = 0.0f;
        return;
    }
    if (begin == end) {
        if (fresh) dst[p] = 1.0f;
        return;
    }
    float cur = fresh ? 1.0f : dst[p];
    for (int i = begin; i < end; i++) {
        const int qi = tile_list[i];
        const QuadRec &r = recs[qi];
        const int ix = x - r.left, iy = y - r.up;
        if ((unsigned)ix >= (unsigned)r.bw || (unsigned)iy >= (unsigned)r.bh) continue;
        if (!vkp::quad_covers(r.e, ix, iy)) continue;
        const bool use_neg = r.quadratic && votes[2 * qi] < votes[2 * qi + 1];      // the positive root wins a tie
        float u, v;
        solve(r, ix, iy, use_neg, r.comp == VKX_QUAD_U, u, v);
        const float value = r.comp == VKX_QUAD_U ? u : v;
        if (!(value > 0.0f)) continue;
        if (mode == VKX_FILL_PLAIN || (mode == VKX_FILL_KEEP_MAX ? cur < value : cur > value)) cur = value;
    }
    dst[p] = cur;
}

// grid: 256 pixels of the bounding box a workgroup
__global__ void __launch_bounds__(256) k_quad_uv(const QuadRec *__restrict__ recs, const int *__restrict__ votes, float2 *__restrict__ uv)
{
    const QuadRec &r = recs[0];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= r.bh * r.bw) return;
    const int iy = idx / r.bw, ix = idx - iy * r.bw;
    float u = 0.0f, v = 0.0f;
    if (vkp::quad_covers(r.e, ix, iy)) solve(r, ix, iy, r.quadratic && votes[0] < votes[1], true, u, v);
    uv[idx] = make_float2(u, v);
}

// grid: the tiles of the masks; boxes {up, left, height, width}, the first n_text the text lines'
__global__ void __launch_bounds__(256) k_box_masks(const int4 *__restrict__ boxes, const int *__restrict__ tile_start,
                                                   const int *__restrict__ tile_list, int n_text, int h, int w, int tiles_x,
                                                   uint8_t *__restrict__ text_mask, uint8_t *__restrict__ boundary_mask,
                                                   uint8_t *__restrict__ both_mask)
{
    int x, y;
    if (!vkd::tile_pixel<kTileW, kTileH>(tiles_x, h, w, x, y)) return;
    bool text = false, dilated = false;
    for (int i = tile_start[blockIdx.x]; i < tile_start[blockIdx.x + 1]; i++) {
        const int bi = tile_list[i];
        const int4 b = boxes[bi];
        if ((unsigned)(y - b.x) < (unsigned)b.z && (unsigned)(x - b.y) < (unsigned)b.w) {
            if (bi < n_text) text = true; else dilated = true;
        }
    }
    const size_t p = (size_t)y * w + x;
    text_mask[p] = text ? 1 : 0;
    if (boundary_mask) boundary_mask[p] = dilated && !text ? 1 : 0;
    if (both_mask) both_mask[p] = dilated || text ? 1 : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// the record of a quad whose bounding box has been checked
void make_rec(const vkx_quad &q, QuadRec &r)
{
    const int xmin = *std::min_element(q.x, q.x + 4), xmax = *std::max_element(q.x, q.x + 4);
    const int ymin = *std::min_element(q.y, q.y + 4), ymax = *std::max_element(q.y, q.y + 4);
    int vx[4], vy[4];
    for (int i = 0; i < 4; i++) { vx[i] = (int)((long long)q.x[i] - xmin); vy[i] = (int)((long long)q.y[i] - ymin); }
    for (int i = 0; i < 4; i++) r.e[i] = vkp::make_edge(vx[(i + 3) & 3], vy[(i + 3) & 3], vx[i], vy[i]);
    r.up = ymin; r.left = xmin;
    r.bh = (int)((long long)ymax - ymin + 1); r.bw = (int)((long long)xmax - xmin + 1);
    r.x0 = q.sx[0]; r.y0 = q.sy[0];
    r.b1x = q.sx[1] - q.sx[0]; r.b1y = q.sy[1] - q.sy[0];
    r.b2x = q.sx[3] - q.sx[0]; r.b2y = q.sy[3] - q.sy[0];
    const float t0x = q.sx[0] - q.sx[1], t0y = q.sy[0] - q.sy[1];
    const float t1x = t0x - q.sx[3], t1y = t0y - q.sy[3];
    r.b3x = t1x + q.sx[2]; r.b3y = t1y + q.sy[2];
    // float32 cross products: each product and the difference rounded
    const float a0 = r.b2x * r.b3y, a1 = r.b2y * r.b3x;
    const float a = a0 - a1;
    const float c0 = r.b1x * r.b2y, c1 = r.b1y * r.b2x;
    r.b1xb2 = c0 - c1;
    r.quadratic = std::fabs((double)a) < 0.001 ? 0 : 1;
    r.four_a = (float)(4.0 * (double)a);
    r.i2a = r.quadratic ? (float)(0.5 / (double)a) : 0.0f;
    r.comp = q.component;
    r.pad = 0;
}

bool box_fits(const int32_t *x, const int32_t *y, long long h, long long w)
{
    for (int i = 0; i < 4; i++)
        if (x[i] < 0 || x[i] >= w || y[i] < 0 || y[i] >= h) return false;
    return true;
}

}  // namespace

VKX_EXPORT int vkx_quad_interp_fill_dev(vkx_ctx *ctx, const vkx_quad *quads_host, int n_quads, int mode, int h, int w, float *dst,
                                        const uint8_t *zero_where)
{
    const int fresh = (mode & VKX_QUAD_FRESH_ONE) ? 1 : 0;
    mode &= ~VKX_QUAD_FRESH_ONE;
    VKX_REQUIRE(ctx && dst, "NULL argument");
    VKX_REQUIRE(n_quads >= 0 && n_quads <= kMaxQuads, "0 .. 2^24 - 1 quads");
    VKX_REQUIRE(n_quads == 0 || quads_host, "NULL argument");
    VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "a plane side outside 1 .. 32768");
    VKX_REQUIRE(mode == VKX_FILL_PLAIN || mode == VKX_FILL_KEEP_MAX || mode == VKX_FILL_KEEP_MIN, "unknown fill mode");
    for (int i = 0; i < n_quads; i++) {
        VKX_REQUIRE(quads_host[i].component == VKX_QUAD_U || quads_host[i].component == VKX_QUAD_V, "unknown component");
        VKX_REQUIRE(box_fits(quads_host[i].x, quads_host[i].y, h, w), "a quad whose bounding box leaves the plane");
    }
    VKX_REQUIRE(!zero_where || !vkx_planes_overlap(dst, 1, 0, (size_t)h * w * sizeof(float), zero_where, 1, 0, (size_t)h * w),
                "dst overlaps zero_where");
    if (n_quads == 0 && !zero_where && !fresh) return VKX_OK;

    std::vector<QuadRec> recs((size_t)n_quads);
    std::vector<VoteRec> voters;
    long long waves = 0;
    for (int i = 0; i < n_quads; i++) {
        make_rec(quads_host[i], recs[i]);
        if (!recs[i].quadratic) continue;
        voters.push_back(VoteRec{i, (int)waves});
        waves += ((long long)recs[i].bh * recs[i].bw + 63) / 64;
        VKX_REQUIRE(waves < 0x7fffffff, "bounding boxes too large in total");
    }
    Bins bins(h, w);
    auto span_of = [&](int i) {
        const QuadRec &r = recs[i];
        return bins.rect(r.up, r.up + r.bh - 1, r.left, r.left + r.bw - 1);
    };
    VKX_REQUIRE(bins.count(n_quads, kMaxEntries, span_of), "too many (quad, tile) pairs");

    // one staged block: records, bins, voters and the zeroed vote counts travel as ONE asynchronous copy
    vkx_tables tab(ctx);
    const size_t r_off = tab.add(sizeof(QuadRec) * std::max<size_t>(recs.size(), 1));
    const size_t s_off = tab.add(sizeof(int) * bins.start.size());
    const size_t l_off = tab.add(sizeof(int) * std::max<size_t>(bins.pairs(), 1));
    const size_t v_off = tab.add(sizeof(VoteRec) * std::max<size_t>(voters.size(), 1));
    const size_t c_off = tab.add(sizeof(int) * 2 * std::max<size_t>(recs.size(), 1));
    int rc;
    if ((rc = tab.take())) return rc;
    if (!recs.empty()) memcpy(tab.at<QuadRec>(r_off), recs.data(), sizeof(QuadRec) * recs.size());
    memcpy(tab.at<int>(s_off), bins.start.data(), sizeof(int) * bins.start.size());
    bins.fill(n_quads, tab.at<int>(l_off), span_of);
    if (!voters.empty()) memcpy(tab.at<VoteRec>(v_off), voters.data(), sizeof(VoteRec) * voters.size());
    memset(tab.at<int>(c_off), 0, sizeof(int) * 2 * std::max<size_t>(recs.size(), 1));
    if ((rc = tab.copy_to(&ctx->quad_tables, (size_t)64 << 10))) return rc;
    unsigned char *base = (unsigned char *)ctx->quad_tables.ptr;
    const QuadRec *d_recs = (const QuadRec *)(base + r_off);
    int *d_votes = (int *)(base + c_off);
    if (waves > 0) {
        { VKX_TIMED(ctx, "k_quad_vote"); k_quad_vote<<<vkx_blocks((size_t)waves, 4), 256, 0, ctx->stream>>>(d_recs, (const VoteRec *)(base + v_off), (int)voters.size(), (int)waves, d_votes); }
        VKX_LAUNCH_CHECK();
    }
    { VKX_TIMED(ctx, "k_quad_fill"); k_quad_fill<<<(unsigned)(bins.tiles_x * bins.tiles_y), 256, 0, ctx->stream>>>(d_recs, (const int *)(base + s_off), (const int *)(base + l_off), d_votes, mode, fresh, h, w, bins.tiles_x, dst, zero_where); }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_quad_interp_uv_dev(vkx_ctx *ctx, const vkx_quad *quad_host, float *uv, size_t uv_floats)
{
    VKX_REQUIRE(ctx && quad_host && uv, "NULL argument");
    const vkx_quad &q = *quad_host;
    VKX_REQUIRE(q.component == VKX_QUAD_U || q.component == VKX_QUAD_V, "unknown component");
    const long long bw = (long long)*std::max_element(q.x, q.x + 4) - *std::min_element(q.x, q.x + 4) + 1;
    const long long bh = (long long)*std::max_element(q.y, q.y + 4) - *std::min_element(q.y, q.y + 4) + 1;
    VKX_REQUIRE(bw <= kMaxSide && bh <= kMaxSide, "a bounding-box side above 32768");
    VKX_REQUIRE(uv_floats == (size_t)(2 * bh * bw), "uv_floats is not 2 * bh * bw");
    QuadRec rec;
    make_rec(q, rec);
    vkx_tables tab(ctx);
    const size_t r_off = tab.add(sizeof(QuadRec));
    const size_t v_off = tab.add(sizeof(VoteRec));
    const size_t c_off = tab.add(sizeof(int) * 2);
    int rc;
    if ((rc = tab.take())) return rc;
    *tab.at<QuadRec>(r_off) = rec;
    *tab.at<VoteRec>(v_off) = VoteRec{0, 0};
    memset(tab.at<int>(c_off), 0, sizeof(int) * 2);
    if ((rc = tab.copy_to(&ctx->quad_tables, (size_t)64 << 10))) return rc;
    unsigned char *base = (unsigned char *)ctx->quad_tables.ptr;
    const QuadRec *d_rec = (const QuadRec *)(base + r_off);
    int *d_votes = (int *)(base + c_off);
    const size_t area = (size_t)(bh * bw);
    if (rec.quadratic) {
        const size_t waves = (area + 63) / 64;
        { VKX_TIMED(ctx, "k_quad_vote"); k_quad_vote<<<vkx_blocks(waves, 4), 256, 0, ctx->stream>>>(d_rec, (const VoteRec *)(base + v_off), 1, (int)waves, d_votes); }
        VKX_LAUNCH_CHECK();
    }
    { VKX_TIMED(ctx, "k_quad_uv"); k_quad_uv<<<vkx_blocks(area, 256), 256, 0, ctx->stream>>>(d_rec, d_votes, (float2 *)uv); }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_box_label_masks_dev(vkx_ctx *ctx, const int32_t *boxes_host, int n_text, int n_dilated, int h, int w,
                                       uint8_t *text_mask, uint8_t *boundary_mask, uint8_t *both_mask)
{
    VKX_REQUIRE(ctx && text_mask, "NULL argument");
    VKX_REQUIRE(n_text >= 0 && n_text <= kMaxQuads && n_dilated >= 0 && n_dilated <= kMaxQuads, "0 .. 2^24 - 1 boxes a list");
    const int n = n_text + n_dilated;
    VKX_REQUIRE(n == 0 || boxes_host, "NULL argument");
    VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "a plane side outside 1 .. 32768");
    for (int i = 0; i < n; i++) {
        const int32_t *b = boxes_host + 4 * (size_t)i;
        VKX_REQUIRE(b[2] >= 1 && b[3] >= 1 && b[0] >= 0 && b[1] >= 0 && b[0] <= h - b[2] && b[1] <= w - b[3], "a box outside the plane");
    }
    const size_t bytes = (size_t)h * w;
    const vkx_plane_bytes planes[3] = {{text_mask, bytes}, {boundary_mask, bytes}, {both_mask, bytes}};
    VKX_REQUIRE(vkx_planes_disjoint(planes, 3), "masks overlap");
    Bins bins(h, w);
    auto span_of = [&](int i) {
        const int32_t *b = boxes_host + 4 * (size_t)i;
        return bins.rect(b[0], b[0] + b[2] - 1, b[1], b[1] + b[3] - 1);
    };
    VKX_REQUIRE(bins.count(n, kMaxEntries, span_of), "too many (box, tile) pairs");
    vkx_tables tab(ctx);
    const size_t b_off = tab.add(sizeof(int32_t) * 4 * std::max(n, 1));
    const size_t s_off = tab.add(sizeof(int) * bins.start.size());
    const size_t l_off = tab.add(sizeof(int) * std::max<size_t>(bins.pairs(), 1));
    int rc;
    if ((rc = tab.take())) return rc;
    if (n) memcpy(tab.at<int32_t>(b_off), boxes_host, sizeof(int32_t) * 4 * (size_t)n);
    memcpy(tab.at<int>(s_off), bins.start.data(), sizeof(int) * bins.start.size());
    bins.fill(n, tab.at<int>(l_off), span_of);
    if ((rc = tab.copy_to(&ctx->quad_tables, (size_t)64 << 10))) return rc;
    const unsigned char *base = (const unsigned char *)ctx->quad_tables.ptr;
    { VKX_TIMED(ctx, "k_box_masks"); k_box_masks<<<(unsigned)(bins.tiles_x * bins.tiles_y), 256, 0, ctx->stream>>>((const int4 *)(base + b_off), (const int *)(base + s_off), (const int *)(base + l_off), n_text, h, w, bins.tiles_x, text_mask, boundary_mask, both_mask); }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
