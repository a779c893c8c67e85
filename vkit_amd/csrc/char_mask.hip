// The external_ellipse char-mask engine on gfx950 (reference: engine/char_mask/external_ellipse.py:104-220).
//
// Per char the reference builds two getPerspectiveTransform matrices, warps a disc template with warpPerspective into the
// char's perspective, trims the result against the page (or a caller box) and fills it into the combined mask.  Here one
// call takes every char of up to 8 sets of one page and paints fresh planes in three launches and one synchronisation:
//   k_char_mask_setup    one lane per char: the two homographies, the placement and the trim, a status for the cases where
//                        the reference raises; the boxes travel to the host (the one synchronisation), which raises or
//                        lays the trimmed boxes out as 16 x 16 tiles (vkb::box_tile_starts);
//   k_char_mask_raster   one workgroup per tile (vkd::box_tile_pixel): the warpPerspective sample of the disc
//                        (vkd::CoordPerspective and vkd::sample_u8, shared with remap.hip) at each pixel; coverage (sample != 0)
//                        takes an atomicMax of the char's rank in the set's ownership plane, and the packed per-char masks take
//                        the sample itself;
//   k_char_mask_resolve  every pixel of every set: mask = owner != 0, score = value of the owner (0 where none), and the
//                        ownership plane back to zero for the next call.
#include "vkx_cell.h"
#include "vkx_internal.h"
#include "vkx_tile_bins.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kTile = 16;                 // tile side: one lane per pixel of a 16 x 16 tile
constexpr int kMaxSets = 8;
constexpr int kMaxSide = 2048;            // internal_side_length limit: the integer disc test equals the float32 one below it

enum { kOk = 0, kShapeMismatch = 1, kEmptyBox = 2, kNotFinite = 3, kTooLarge = 4 };

struct CharIn {            // one char as the host stages it
    double q[8];           // smooth (x, y) of the 4 points
    int bounds[4];         // up, down, left, right: the page or the caller's box
    float value;           // score of the char (score planes)
    int set;
    int rank;              // 1-based position in its set: the later char wins the score
    int pad;
};

struct CharGeo {           // what the setup pass leaves for the raster
    vkd::CoordPerspective coord;
    int up, left, bh, bw;  // the trimmed box in page coordinates
    int mat_up, mat_left;  // ... and its origin inside the warped template
    int status;
    int pad;
};

struct SetDev {
    uint8_t *mask;
    float *score;
    uint8_t *packed;       // per-char masks, row-major one after the other, or NULL
    int *owner;
    int first;             // first char of the set in the global table
    int n;
};

// The disc template build_np_distance(R) <= R (engine/char_heatmap/default.py:30-40), read through sample_u8 as if it
// were an E x E uint8 plane: sqrt(dy^2 + dx^2) <= R in float32 is dy^2 + dx^2 <= R^2 for R < 2048 (the squares are exact,
// and sqrt(R^2 + 1) rounds above R).
struct DiscPtr {
    int R, E;
    ptrdiff_t off;
    __device__ __forceinline__ DiscPtr operator+(ptrdiff_t d) const { return DiscPtr{R, E, off + d}; }
    __device__ __forceinline__ int operator[](ptrdiff_t k) const
    {
        const int i = (int)(off + k), y = i / E, x = i - y * E;
        const int dy = y - R, dx = x - R;
        return dy * dy + dx * dx <= R * R;
    }
};

// numpy min / max of 4 float64 values: NaN wins
__device__ inline double nan_min4(const double v[4])
{
    double r = v[0];
    for (int i = 1; i < 4; i++) r = (isnan(r) || v[i] >= r) ? r : v[i];
    for (int i = 0; i < 4; i++) if (isnan(v[i])) r = v[i];
    return r;
}
__device__ inline float nan_max4f(const float v[4])
{
    float r = v[0];
    for (int i = 1; i < 4; i++) r = v[i] > r ? v[i] : r;
    for (int i = 0; i < 4; i++) if (isnan(v[i])) r = v[i];
    return r;
}

// len(range(n)[a:b]) for a >= 0 (Python slice semantics: a negative b counts from the end)
__device__ inline long long slice_len(long long n, long long a, long long b)
{
    if (b < 0) { b += n; if (b < 0) b = 0; } else if (b > n) b = n;
    if (a > n) a = n;
    return b > a ? b - a : 0;
}

__device__ inline bool ceil_to_int(float v, long long &out, int &status)
{
    if (isnan(v)) { status = kNotFinite; return false; }
    if (!(fabsf(v) < 1073741824.f)) { status = kTooLarge; return false; }
    out = (long long)ceilf(v);
    return true;
}

__global__ void __launch_bounds__(256) k_char_mask_setup(const CharIn *__restrict__ chars, int n, int L, int R, CharGeo *__restrict__ geo,
                                                         int *__restrict__ boxes)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const CharIn c = chars[g];
    const int E = 2 * R + 1, pad = (E - L) / 2;
    const float cb = (float)pad, ce = (float)(pad + L - 1), ee = (float)(E - 1);
    const float char_pts[8] = {cb, cb, ce, cb, ce, ce, cb, ce};
    const float ext_pts[8] = {0.f, 0.f, ee, 0.f, ee, ee, 0.f, ee};
    int status = kOk;
    CharGeo G;
    G.up = G.left = G.bh = G.bw = G.mat_up = G.mat_left = 0;
    G.pad = 0;
    int out_box[4] = {0, -1, 0, -1};

    // 1. H1: char points -> the polygon's self-relative points (Polygon.internals)
    float rel[8];
    vkc::quad_internals(c.q, rel);
    double H[9];
    vkc::perspective_transform(char_pts, rel, H);

    // affine_np_points of the four external points (four columns)
    double px[4], py[4];
    for (int k = 0; k < 4; k++) vkc::affine_point(H, ext_pts[2 * k], ext_pts[2 * k + 1], false, px[k], py[k]);
    const double y_off = nan_min4(py), x_off = nan_min4(px);
    float tp[8], tx[4], ty[4];
    for (int k = 0; k < 4; k++) {
        tx[k] = (float)(px[k] - x_off);
        ty[k] = (float)(py[k] - y_off);
        tp[2 * k] = tx[k];
        tp[2 * k + 1] = ty[k];
    }
    // 2. H2: external points -> those; the warp's size is (ceil(x max), ceil(y max))
    double H2[9];
    vkc::perspective_transform(ext_pts, tp, H2);
    long long th = 0, tw = 0;
    if (ceil_to_int(nan_max4f(ty), th, status) && ceil_to_int(nan_max4f(tx), tw, status)) {
        // 3. placement: round(min smooth + offset), Python's round (halves to even)
        double sy = c.q[1], sx = c.q[0];
        for (int k = 1; k < 4; k++) { sy = fmin(sy, c.q[2 * k + 1]); sx = fmin(sx, c.q[2 * k]); }
        const double fu = rint(sy + y_off), fl = rint(sx + x_off);
        if (!(fabs(fu) < 1073741824.0) || !(fabs(fl) < 1073741824.0)) {
            status = isnan(fu) || isnan(fl) ? kNotFinite : kTooLarge;
        } else {
            long long up = (long long)fu, left = (long long)fl;
            long long down = up + th - 1, right = left + tw - 1;
            long long tu = 0, td = th - 1, tl = 0, tr = tw - 1;
            if (up < c.bounds[0]) { tu = c.bounds[0] - up; up = c.bounds[0]; }
            if (down > c.bounds[1]) { td -= down - c.bounds[1]; down = c.bounds[1]; }
            if (left < c.bounds[2]) { tl = c.bounds[2] - left; left = c.bounds[2]; }
            if (right > c.bounds[3]) { tr -= right - c.bounds[3]; right = c.bounds[3]; }
            // cv.warpPerspective takes the source size for a dsize with a zero side
            const long long mh = (th > 0 && tw > 0) ? th : E, mw = (th > 0 && tw > 0) ? tw : E;
            const long long bh = down - up + 1, bw = right - left + 1;
            if (slice_len(mh, tu, td + 1) != bh || slice_len(mw, tl, tr + 1) != bw) status = kShapeMismatch;   // Mask(box=...)
            else if (bh == 0 || bw == 0) status = kEmptyBox;                                                   // Box.extract_np_array
            if (status == kOk) {
                G.coord = vkd::make_perspective(H2, (int)th, (int)tw);
                G.up = (int)up; G.left = (int)left; G.bh = (int)bh; G.bw = (int)bw;
                G.mat_up = (int)tu; G.mat_left = (int)tl;
            }
            out_box[0] = (int)up; out_box[1] = (int)down; out_box[2] = (int)left; out_box[3] = (int)right;
        }
    }
    G.status = status;
    geo[g] = G;
    int *b = boxes + (size_t)g * 5;
    for (int i = 0; i < 4; i++) b[i] = status == kOk ? out_box[i] : 0;
    b[4] = status;
}

// one workgroup per 16 x 16 tile of a trimmed char box; tile_start[g] .. tile_start[g + 1] are char g's tiles
__global__ void __launch_bounds__(256) k_char_mask_raster(const CharIn *__restrict__ chars, const CharGeo *__restrict__ geo,
                                                          const int *__restrict__ tile_start, const long long *__restrict__ packed_off,
                                                          int n, int R, int w, const SetDev *__restrict__ sets)
{
    int rx, ry;
    const int lo = vkd::box_tile_pixel<kTile, kTile>(n, tile_start, [&](int g) { return geo[g].bw; }, rx, ry);     // the char of the tile
    const CharGeo &G = geo[lo];
    if (ry >= G.bh || rx >= G.bw) return;
    const int E = 2 * R + 1;
    int X, Y;
    G.coord(G.mat_left + rx, G.mat_up + ry, X, Y);
    uint8_t v;
    vkd::sample_u8<1, DiscPtr>(DiscPtr{R, E, 0}, E, E, E, X, Y, &v);
    const SetDev &S = sets[chars[lo].set];
    if (S.packed) S.packed[packed_off[lo] + (ptrdiff_t)ry * G.bw + rx] = v;
    if (v && S.owner) atomicMax(S.owner + (ptrdiff_t)(G.up + ry) * w + (G.left + rx), chars[lo].rank);
}

// grid (pixels / 256, 1, n_sets)
__global__ void __launch_bounds__(256) k_char_mask_resolve(const CharIn *__restrict__ chars, const SetDev *__restrict__ sets,
                                                           size_t page)
{
    const SetDev S = sets[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= page || !S.owner) return;
    const int o = S.owner[i];
    if (S.mask) S.mask[i] = o != 0;
    if (S.score) S.score[i] = o ? chars[S.first + o - 1].value : 0.f;
    if (o) S.owner[i] = 0;
}

// Argument checks shared by both forms.
int check_sets(const vkx_char_set *sets, int n_sets, int L, int h, int w, long long *total)
{
    VKX_REQUIRE(sets || n_sets == 0, "NULL argument");
    VKX_REQUIRE(n_sets >= 0 && n_sets <= kMaxSets, "0 .. 8 sets");
    VKX_REQUIRE(L >= 1 && L <= kMaxSide, "internal_side_length 1 .. 2048");
    VKX_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < (1LL << 31), "bad page shape");
    long long n = 0;
    std::vector<vkx_plane_bytes> outs;
    for (int s = 0; s < n_sets; s++) {
        const vkx_char_set &S = sets[s];
        VKX_REQUIRE(S.n_chars >= 0, "negative char count");
        VKX_REQUIRE(S.n_chars == 0 || (S.pts_host && S.poly_offsets_host && S.boxes_host), "NULL char table");
        VKX_REQUIRE(!S.score || S.values_host || S.n_chars == 0, "a score plane needs values");
        VKX_REQUIRE(!S.char_masks || S.char_masks_cap >= 0, "negative char mask capacity");
        for (int i = 0; i < S.n_chars; i++) {
            VKX_REQUIRE(S.poly_offsets_host[i + 1] - S.poly_offsets_host[i] == 4, "a char polygon has exactly 4 points");
            const double *q = S.pts_host + 2 * (size_t)S.poly_offsets_host[i];
            for (int k = 0; k < 8; k++) VKX_REQUIRE(std::isfinite(q[k]), "non-finite char point");
            if (S.bounds_host) {
                const int *b = S.bounds_host + 4 * (size_t)i;
                VKX_REQUIRE(0 <= b[0] && b[0] <= b[1] && b[1] < h && 0 <= b[2] && b[2] <= b[3] && b[3] < w,
                            "a bounding box outside the page");
            }
        }
        VKX_REQUIRE(S.n_chars == 0 || S.poly_offsets_host[0] == 0, "offsets start at 0");
        if (S.mask) outs.push_back({S.mask, (size_t)h * w});
        if (S.score) outs.push_back({S.score, (size_t)h * w * 4});
        if (S.char_masks && S.char_masks_cap) outs.push_back({S.char_masks, (size_t)S.char_masks_cap});
        n += S.n_chars;
    }
    VKX_REQUIRE(vkx_planes_disjoint(outs.data(), outs.size()), "output planes overlap");
    VKX_REQUIRE(n < (1LL << 24), "at most 2^24 chars");
    *total = n;
    return VKX_OK;
}

}  // namespace

VKX_EXPORT int vkx_char_mask_ellipse_sets_fresh_dev(vkx_ctx *ctx, int internal_side_length, const vkx_char_set *sets, int n_sets,
                                                    int h, int w)
{
    VKX_REQUIRE(ctx, "NULL argument");
    const int L = internal_side_length;
    long long total = 0;
    int rc = check_sets(sets, n_sets, L, h, w, &total);
    if (rc) return rc;
    if (n_sets == 0) return VKX_OK;
    const int n = (int)total;
    const int R = (int)std::ceil(L / std::sqrt(2.0));       // math.ceil(L / math.sqrt(2))

    // the char table, in set order, written where it is staged
    vkx_tables tab(ctx);
    tab.add(sizeof(CharIn) * (size_t)std::max(n, 1));
    if ((rc = tab.take())) return rc;
    CharIn *table = tab.at<CharIn>(0);
    if (!n) table[0] = CharIn();
    std::vector<int> firsts(n_sets);
    int g = 0;
    for (int s = 0; s < n_sets; s++) {
        const vkx_char_set &S = sets[s];
        firsts[s] = g;
        for (int i = 0; i < S.n_chars; i++, g++) {
            CharIn &c = table[g];
            memcpy(c.q, S.pts_host + 2 * (size_t)S.poly_offsets_host[i], sizeof(c.q));
            if (S.bounds_host) memcpy(c.bounds, S.bounds_host + 4 * (size_t)i, sizeof(c.bounds));
            else { c.bounds[0] = 0; c.bounds[1] = h - 1; c.bounds[2] = 0; c.bounds[3] = w - 1; }
            c.value = S.score ? S.values_host[i] : 0.f;
            c.set = s;
            c.rank = i + 1;
            c.pad = 0;
        }
    }
    const size_t page = (size_t)h * w;
    const size_t geo_bytes = vkx_align256(sizeof(CharGeo) * (size_t)n);
    const size_t box_bytes = vkx_align256(sizeof(int) * 5 * (size_t)n);
    if ((rc = vkx_scratch_reserve(ctx, &ctx->char_geo, std::max(geo_bytes + box_bytes, (size_t)64 << 10)))) return rc;
    CharGeo *geo = (CharGeo *)ctx->char_geo.ptr;
    int *boxes = (int *)((char *)ctx->char_geo.ptr + geo_bytes);
    if ((rc = tab.copy_to(&ctx->char_table, (size_t)64 << 10))) return rc;
    const CharIn *chars = (const CharIn *)ctx->char_table.ptr;

    // 1. setup, then the boxes and statuses to the host: the call's one synchronisation
    std::vector<int> host_boxes((size_t)5 * std::max(n, 1));
    if (n) {
        {
            VKX_TIMED(ctx, "k_char_mask_setup");
            k_char_mask_setup<<<vkx_blocks(n, 256), 256, 0, ctx->stream>>>(chars, n, L, R, geo, boxes);
        }
        VKX_LAUNCH_CHECK();
        vkx_device_guard guard(ctx);
        VKX_HIP(hipMemcpyAsync(host_boxes.data(), boxes, sizeof(int) * 5 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        VKX_HIP(hipStreamSynchronize(ctx->stream));
    }
    bool failed = false;
    for (int s = 0, k = 0; s < n_sets; s++) {
        memcpy(sets[s].boxes_host, host_boxes.data() + (size_t)5 * k, sizeof(int) * 5 * (size_t)sets[s].n_chars);
        for (int i = 0; i < sets[s].n_chars; i++, k++) failed = failed || host_boxes[(size_t)5 * k + 4] != kOk;
    }
    if (failed) return VKX_ERR_CHAR_MASK;      // the reference raises: no plane written

    // 2. the tile and packed-mask layout
    auto box_sides = [&](int k, long long &bh, long long &bw) {
        const int *b = host_boxes.data() + (size_t)5 * k;
        bh = b[1] - b[0] + 1;
        bw = b[3] - b[2] + 1;
    };
    std::vector<long long> packed((size_t)std::max(n, 1));
    for (int s = 0, k = 0; s < n_sets; s++) {
        long long off = 0;
        for (int i = 0; i < sets[s].n_chars; i++, k++) {
            long long bh, bw;
            box_sides(k, bh, bw);
            packed[k] = off;
            off += bh * bw;
        }
        if (sets[s].char_masks) VKX_REQUIRE(off <= sets[s].char_masks_cap, "char mask buffer too small for the packed masks");
    }
    std::vector<int> tile_start;
    VKX_REQUIRE((vkb::box_tile_starts<kTile, kTile>(n, box_sides, tile_start)), "too many tiles");
    const int tiles = tile_start[n];

    // 3. the ownership planes (all zero between calls: the resolve clears what it reads)
    const size_t owner_bytes = sizeof(int) * page * n_sets;
    if (owner_bytes > ctx->char_owner.cap) ctx->char_owner_zeroed = 0;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->char_owner, owner_bytes))) return rc;
    {
        vkx_device_guard guard(ctx);
        if (ctx->char_owner_zeroed < owner_bytes) VKX_HIP(hipMemsetAsync(ctx->char_owner.ptr, 0, ctx->char_owner.cap, ctx->stream));
    }
    ctx->char_owner_zeroed = 0;
    // one staged block: sets, tile starts, packed offsets
    vkx_tables lay(ctx);
    const size_t sets_off = lay.add(sizeof(SetDev) * kMaxSets), ts_off = lay.add(sizeof(int) * tile_start.size());
    const size_t packed_off = lay.add(sizeof(long long) * packed.size());
    if ((rc = lay.take())) return rc;
    SetDev *sd = lay.at<SetDev>(sets_off);
    for (int s = 0; s < n_sets; s++) {
        sd[s].mask = sets[s].mask;
        sd[s].score = sets[s].score;
        sd[s].packed = sets[s].char_masks;
        sd[s].owner = (int *)ctx->char_owner.ptr + page * s;
        sd[s].first = firsts[s];
        sd[s].n = sets[s].n_chars;
    }
    memcpy(lay.at<int>(ts_off), tile_start.data(), sizeof(int) * tile_start.size());
    memcpy(lay.at<long long>(packed_off), packed.data(), sizeof(long long) * packed.size());
    if ((rc = lay.copy_to(&ctx->char_layout, (size_t)64 << 10))) return rc;
    const SetDev *sets_dev = (const SetDev *)((char *)ctx->char_layout.ptr + sets_off);
    const int *tile_dev = (const int *)((char *)ctx->char_layout.ptr + ts_off);
    const long long *packed_dev = (const long long *)((char *)ctx->char_layout.ptr + packed_off);

    if (tiles) {
        VKX_TIMED(ctx, "k_char_mask_raster");
        k_char_mask_raster<<<(unsigned)tiles, 256, 0, ctx->stream>>>(chars, geo, tile_dev, packed_dev, n, R, w, sets_dev);
    }
    VKX_LAUNCH_CHECK();
    {
        VKX_TIMED(ctx, "k_char_mask_resolve");
        k_char_mask_resolve<<<dim3(vkx_blocks(page, 256), 1, n_sets), 256, 0, ctx->stream>>>(chars, sets_dev, page);
    }
    VKX_LAUNCH_CHECK();
    ctx->char_owner_zeroed = ctx->char_owner.cap;
    return VKX_OK;
}

// The host form: planes and packed masks in host memory, staged through device scratch; returns after the copies back.
VKX_EXPORT int vkx_char_mask_ellipse_sets_fresh(vkx_ctx *ctx, int internal_side_length, const vkx_char_set *sets, int n_sets,
                                                int h, int w)
{
    VKX_REQUIRE(ctx, "NULL argument");
    long long total = 0;
    int rc = check_sets(sets, n_sets, internal_side_length, h, w, &total);
    if (rc) return rc;
    if (n_sets == 0) return VKX_OK;
    const size_t page = (size_t)h * w;
    size_t bytes = 0;
    std::vector<size_t> at(3 * n_sets);
    for (int s = 0; s < n_sets; s++) {
        at[3 * s] = bytes;
        bytes += sets[s].mask ? vkx_align256(page) : 0;
        at[3 * s + 1] = bytes;
        bytes += sets[s].score ? vkx_align256(4 * page) : 0;
        at[3 * s + 2] = bytes;
        bytes += sets[s].char_masks ? vkx_align256((size_t)sets[s].char_masks_cap) : 0;
    }
    if ((rc = vkx_scratch_reserve(ctx, &ctx->char_host, std::max(bytes, (size_t)256)))) return rc;
    char *base = (char *)ctx->char_host.ptr;
    std::vector<vkx_char_set> dev(sets, sets + n_sets);
    for (int s = 0; s < n_sets; s++) {
        if (dev[s].mask) dev[s].mask = (uint8_t *)(base + at[3 * s]);
        if (dev[s].score) dev[s].score = (float *)(base + at[3 * s + 1]);
        if (dev[s].char_masks) dev[s].char_masks = (uint8_t *)(base + at[3 * s + 2]);
    }
    if ((rc = vkx_char_mask_ellipse_sets_fresh_dev(ctx, internal_side_length, dev.data(), n_sets, h, w))) return rc;
    vkx_device_guard guard(ctx);
    for (int s = 0; s < n_sets; s++) {
        if (sets[s].mask) VKX_HIP(hipMemcpyAsync(sets[s].mask, dev[s].mask, page, hipMemcpyDeviceToHost, ctx->stream));
        if (sets[s].score) VKX_HIP(hipMemcpyAsync(sets[s].score, dev[s].score, 4 * page, hipMemcpyDeviceToHost, ctx->stream));
        if (sets[s].char_masks && sets[s].char_masks_cap)
            VKX_HIP(hipMemcpyAsync(sets[s].char_masks, dev[s].char_masks, (size_t)sets[s].char_masks_cap, hipMemcpyDeviceToHost,
                                   ctx->stream));
    }
    VKX_HIP(hipStreamSynchronize(ctx->stream));
    return VKX_OK;
}
