// The pixel half of render_text_line_meta on gfx950 (reference: vkit/engine/font/freetype.py:314-380 the paste, :600-837 resize,
// pad, trim and the clean-up of a trimmed char's residual pixels).
//
// A page has 50 - 300 text lines of tens of pixels in height.  Composed from the single-plane operations a line is a few launches a
// CHAR (three pastes) plus three resizes; here one call takes EVERY line of a page, its records, resize tables and glyph planes
// staged as one block (vkx_tables, one copy out of the ring), in TWO launches and without a synchronisation.  Every geometric
// decision (char boxes, resized shape, pad, trim index) is the caller's and independent of any pixel; every pixel is the call's:
//   k_text_paste    one lane a pixel of the pasted plane: over the chars of its line (their records in LDS) the last glyph whose
//                   image > 0 gives the colour (the glyph colour; for an LCD glyph the gamma-1 table or the caller's gamma plane), any glyph
//                   sets the mask, the score is the maximum over the char BOXES (`mat < value` of fill_np_array).  A line that is
//                   not resized goes straight into its output at the pad offset (pad pixels 255 / 0 / 0.0) through the clean-up;
//                   a line that is resized goes into context scratch.
//   k_text_resize   one lane an output pixel of a resized line: the pixel of vkx_resize_pixel.h the line's plan names on the three
//                   scratch planes (image u8c3; mask as (m * 255) resized, > 0; score map float32 clipped to [0, 1]), then the
//                   clean-up.  Only what survives the trim is computed.
// The clean-up (horizontal lines, :693-731) is a function of the pixel alone, so both kernels end with it instead of a third
// launch reading the planes back: inside the first trimmed char's box, where that glyph's mask (resized to the box with the
// line's interpolation when the shapes differ) is set the image is 255 and the mask 0, and the score is 0; then inside the last
// kept char's box the score is raised to that glyph's score map (resized likewise, clipped to [0, 1] then).
// The planes are a few kilobytes: the call is bound by launches and latency, not by bandwidth.
#include "vkx_internal.h"
#include "vkx_resize_pixel.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace {

constexpr int kMaxChars = 65536, kMaxLines = 4096;
constexpr int kMaxSide = 32767;
constexpr int kLdsChars = 64;                   // char records a workgroup holds at a time

struct CharRec {
    const uint8_t *image;                       // [gh][gw][cn of its line]
    const float *score;                         // [gh][gw] or NULL
    const uint8_t *paste;                       // [gh][gw][3]: what an LCD glyph pastes, or NULL (the gamma-1 table)
    int gh, gw, up, left;                       // the box in the pasted plane has the glyph's shape
};

struct LineRec {
    int cn, color[3];
    int ph, pw;                                 // the pasted plane
    int pad_up, pad_left, oh, ow;               // the (resized) plane sits at the pad offset of the padded plane; the output is its top left
    int first_char, n_chars, resized, has_score;
    uint8_t *img, *msk;                         // outputs
    float *scr;
    uint8_t *s_img, *s_msk;                     // the pasted planes of a resized line (scratch)
    float *s_scr;
    vkd::PlannedResize r_u8, r_f32;             // the line's resize on uint8 (image, mask) and float32 (score map)
    int cleanup, t_char, k_char;                // the first trimmed and the last kept char (indices of the char table)
    int tb[4], kb[4];                           // their boxes in the padded plane: up, left, height, width
    vkd::PlannedResize r_t, r_k;                // the trimmed glyph's mask -> its box (uint8); the kept glyph's score map -> its box
};

struct TileJob { int line, first_block; };      // the 64 x 4 tiles of a line's domain start at first_block

// What an LCD glyph pastes at gamma 1 (reference :362-366): ((1 - v / 255.0) * 255).astype(uint8) in float64, as numpy computes it.
// That is NOT 255 - v: 1 - v / 255.0 rounds, and for 50 of the 256 values the product falls just below the integer (v = 43 gives
// 211.99999999999997, truncated to 211).  The 256 values are formed on the host, where the three operations are the ones numpy
// runs, and travel with the tables (formed on the device the same expression gave 11 where numpy has 10 for v = 244).
void fill_lcd_values(uint8_t *out)
{
    for (int v = 0; v < 256; v++) {
        const double ratio = (double)v / 255.0;
        const double rest = 1.0 - ratio;
        out[v] = (uint8_t)(int)(rest * 255.0);
    }
}

// (glyph > 0) * 255, any channel of an LCD glyph: CharGlyph.get_glyph_mask through Mask.to_resized_mask's scaling
__device__ __forceinline__ int glyph_ink(const CharRec &g, int cn, int y, int x)
{
    const uint8_t *q = g.image + ((ptrdiff_t)y * g.gw + x) * cn;
    return (cn == 1 ? q[0] : (q[0] | q[1] | q[2])) ? 255 : 0;
}

// The residual pixels of the first trimmed char at padded-plane pixel (y, x) of line L (reference :693-731)
__device__ void cleanup_pixel(const LineRec &L, const CharRec *__restrict__ chars, const unsigned char *tabs, int y, int x,
                              uint8_t img[3], uint8_t &m, float &s)
{
    const int ty = y - L.tb[0], tx = x - L.tb[1];
    if ((unsigned)ty < (unsigned)L.tb[2] && (unsigned)tx < (unsigned)L.tb[3]) {
        const CharRec t = chars[L.t_char];
        uint8_t ink;
        const int cn = L.cn;
        vkd::planned_pixel_u8<1>(L.r_t, tabs, ty, tx, [&](int yy, int xx) { return glyph_ink(t, cn, yy, xx); }, &ink);
        if (ink > 0) { img[0] = img[1] = img[2] = 255; m = 0; }
        if (L.has_score) s = 0.f;
    }
    if (!L.has_score) return;
    const int ky = y - L.kb[0], kx = x - L.kb[1];
    if ((unsigned)ky < (unsigned)L.kb[2] && (unsigned)kx < (unsigned)L.kb[3]) {
        const CharRec k = chars[L.k_char];
        const float q = vkd::planned_pixel_f32(L.r_k, tabs, ky, kx, [&](int yy, int xx) { return k.score[(ptrdiff_t)yy * k.gw + xx]; });
        if (s < q) s = q;                       // keep_max_value: np.putmask(mat, mat < value, value)
    }
}

__device__ __forceinline__ void store_pixel(const LineRec &L, int y, int x, const uint8_t img[3], uint8_t m, float s)
{
    const ptrdiff_t at = (ptrdiff_t)y * L.ow + x;
    uint8_t *o = L.img + 3 * at;
    o[0] = img[0]; o[1] = img[1]; o[2] = img[2];
    L.msk[at] = m;
    if (L.has_score) L.scr[at] = s;
}

// the line of a workgroup of either grid: its tile job, and the workgroup's 64 x 4 tile of the domain width_of(L) wide
template <class WidthOf>
__device__ __forceinline__ const LineRec &line_tile_pixel(const LineRec *lines, const TileJob *jobs, int n_jobs, WidthOf width_of, int &x, int &y)
{
    const int j = vkd::box_tile_pixel<64, 4>(n_jobs, [&](int i) { return jobs[i].first_block; }, [&](int i) { return width_of(lines[jobs[i].line]); }, x, y);
    return lines[jobs[j].line];
}

// grid: the 64 x 4 tiles of every line's domain -- the pasted plane of a resized line, the output of any other
__global__ void __launch_bounds__(256) k_text_paste(const LineRec *__restrict__ lines, const CharRec *__restrict__ chars,
                                                    const TileJob *__restrict__ jobs, int n_jobs, const unsigned char *__restrict__ tabs,
                                                    const uint8_t *__restrict__ lcd_values)
{
    __shared__ CharRec held[kLdsChars];
    if (n_jobs == 0) return;
    int x, y;
    const LineRec &L = line_tile_pixel(lines, jobs, n_jobs, [](const LineRec &l) { return l.resized ? l.pw : l.ow; }, x, y);
    const int dom_h = L.resized ? L.ph : L.oh, dom_w = L.resized ? L.pw : L.ow;
    const bool live = x < dom_w && y < dom_h;
    // the pixel of the pasted plane this lane forms
    const int py = L.resized ? y : y - L.pad_up, px = L.resized ? x : x - L.pad_left;
    const bool inside = live && (unsigned)py < (unsigned)L.ph && (unsigned)px < (unsigned)L.pw;
    const int cn = L.cn;
    uint8_t img[3] = {255, 255, 255}, m = 0;
    float s = 0.f;                              // ScoreMap.from_shape
    for (int first = 0; first < L.n_chars; first += kLdsChars) {
        const int n = min(kLdsChars, L.n_chars - first);
        __syncthreads();
        if ((int)threadIdx.x < n) held[threadIdx.x] = chars[L.first_char + first + threadIdx.x];
        __syncthreads();
        if (!inside) continue;
        for (int c = 0; c < n; c++) {
            const CharRec &g = held[c];
            const int gy = py - g.up, gx = px - g.left;
            if ((unsigned)gy >= (unsigned)g.gh || (unsigned)gx >= (unsigned)g.gw) continue;
            const ptrdiff_t at = (ptrdiff_t)gy * g.gw + gx;
            if (cn == 1) {
                if (g.image[at]) { img[0] = (uint8_t)L.color[0]; img[1] = (uint8_t)L.color[1]; img[2] = (uint8_t)L.color[2]; m = 1; }
                const float q = g.score[at];
                if (s < q) s = q;               // over the whole box, keeping the maximum
            } else {
                const uint8_t *q = g.image + 3 * at;
                if (q[0] | q[1] | q[2]) {
                    if (g.paste) { const uint8_t *v = g.paste + 3 * at; img[0] = v[0]; img[1] = v[1]; img[2] = v[2]; }
                    else { img[0] = lcd_values[q[0]]; img[1] = lcd_values[q[1]]; img[2] = lcd_values[q[2]]; }
                    m = 1;
                }
            }
        }
    }
    if (!live) return;
    if (L.resized) {
        const ptrdiff_t at = (ptrdiff_t)y * L.pw + x;
        uint8_t *o = L.s_img + 3 * at;
        o[0] = img[0]; o[1] = img[1]; o[2] = img[2];
        L.s_msk[at] = m;
        if (L.has_score) L.s_scr[at] = s;
        return;
    }
    if (L.cleanup) cleanup_pixel(L, chars, tabs, y, x, img, m, s);
    store_pixel(L, y, x, img, m, s);
}

// grid: the 64 x 4 tiles of the output of every resized line
__global__ void __launch_bounds__(256) k_text_resize(const LineRec *__restrict__ lines, const CharRec *__restrict__ chars,
                                                     const TileJob *__restrict__ jobs, int n_jobs, const unsigned char *__restrict__ tabs)
{
    if (n_jobs == 0) return;
    int x, y;
    const LineRec &L = line_tile_pixel(lines, jobs, n_jobs, [](const LineRec &l) { return l.ow; }, x, y);
    if (x >= L.ow || y >= L.oh) return;
    uint8_t img[3] = {255, 255, 255}, m = 0;
    float s = 0.f;
    const int ry = y - L.pad_up, rx = x - L.pad_left;
    if ((unsigned)ry < (unsigned)L.r_u8.dh && (unsigned)rx < (unsigned)L.r_u8.dw) {
        const uint8_t *s_img = L.s_img, *s_msk = L.s_msk;
        const float *s_scr = L.s_scr;
        const int pw = L.pw;
        vkd::planned_pixel_u8<3>(L.r_u8, tabs, ry, rx, [&](int yy, int b) { return (int)s_img[(ptrdiff_t)yy * 3 * pw + b]; }, img);
        uint8_t ink;                            // Mask.to_resized_mask: (mask * 255) resized, > 0
        vkd::planned_pixel_u8<1>(L.r_u8, tabs, ry, rx, [&](int yy, int xx) { return s_msk[(ptrdiff_t)yy * pw + xx] ? 255 : 0; }, &ink);
        m = ink > 0 ? 1 : 0;
        if (L.has_score) s = vkd::planned_pixel_f32(L.r_f32, tabs, ry, rx, [&](int yy, int xx) { return s_scr[(ptrdiff_t)yy * pw + xx]; });
    }
    if (L.cleanup) cleanup_pixel(L, chars, tabs, y, x, img, m, s);
    store_pixel(L, y, x, img, m, s);
}

}  // namespace

VKX_EXPORT int vkx_text_lines_dev(vkx_ctx *ctx, const vkx_text_char *chars_host, int n_chars, const vkx_text_line *lines_host, int n_lines,
                                  const void *blob_host, size_t blob_bytes, uint8_t *dst, size_t dst_bytes)
{
    VKX_REQUIRE(n_chars >= 1 && n_chars <= kMaxChars, "1 .. 65536 chars");
    VKX_REQUIRE(n_lines >= 1 && n_lines <= kMaxLines, "1 .. 4096 lines");
    VKX_REQUIRE(ctx && chars_host && lines_host && blob_host && dst, "NULL argument");
    VKX_REQUIRE(blob_bytes <= ((size_t)1 << 30) && dst_bytes <= ((size_t)1 << 40), "blob beyond 2^30 or dst beyond 2^40 bytes");
    VKX_REQUIRE((uintptr_t)dst % 4 == 0, "dst not aligned to 4 bytes");

    auto in_blob = [&](long long off, size_t bytes) { return off >= 0 && (unsigned long long)off <= blob_bytes && bytes <= blob_bytes - (size_t)off; };

    std::vector<LineRec> lines(n_lines);
    std::vector<CharRec> chars(n_chars);
    std::vector<TileJob> paste_jobs(n_lines), resize_jobs;
    vkd::ResizePlanner planner(__func__);
    std::vector<std::pair<long long, long long>> ranges;
    long long paste_blocks = 0, resize_blocks = 0, scratch_bytes = 0;

    // the first and the number of chars of every line: the chars of a line are consecutive (ascending `line`)
    std::vector<int> first_char(n_lines, 0), count(n_lines, 0);
    for (int i = 0; i < n_chars; i++) {
        const int line = chars_host[i].line;
        VKX_REQUIRE(line >= 0 && line < n_lines, "line index outside the table");
        VKX_REQUIRE(i == 0 || line >= chars_host[i - 1].line, "chars not grouped by ascending line");
        if (count[line]++ == 0) first_char[line] = i;
    }

    for (int i = 0; i < n_lines; i++) {
        const vkx_text_line &p = lines_host[i];
        LineRec &L = lines[i];
        VKX_REQUIRE(p.channels == 1 || p.channels == 3, "a line has glyphs of 1 or of 3 channels");
        VKX_REQUIRE(count[i] >= 1, "a line without chars");
        for (int c = 0; c < 3; c++) VKX_REQUIRE(p.color[c] >= 0 && p.color[c] <= 255, "glyph colour outside 0 .. 255");
        VKX_REQUIRE(p.paste_h >= 1 && p.paste_w >= 1 && p.paste_h <= kMaxSide && p.paste_w <= kMaxSide, "pasted plane side outside 1 .. 32767");
        VKX_REQUIRE(p.resized_h >= 1 && p.resized_w >= 1 && p.resized_h <= kMaxSide && p.resized_w <= kMaxSide, "resized plane side outside 1 .. 32767");
        VKX_REQUIRE(p.out_h >= 1 && p.out_w >= 1 && p.out_h <= kMaxSide && p.out_w <= kMaxSide, "output side outside 1 .. 32767");
        VKX_REQUIRE(p.pad_up >= 0 && p.pad_left >= 0 && p.pad_up <= kMaxSide && p.pad_left <= kMaxSide, "pad outside 0 .. 32767");
        VKX_REQUIRE(vkd::ResizePlanner::known_interpolation(p.interpolation), "unknown interpolation code");
        VKX_REQUIRE((p.has_score != 0) == (p.channels == 1), "a 1-channel line has a score map, an LCD line has none");
        L.cn = p.channels;
        for (int c = 0; c < 3; c++) L.color[c] = p.color[c];
        L.ph = p.paste_h; L.pw = p.paste_w; L.pad_up = p.pad_up; L.pad_left = p.pad_left; L.oh = p.out_h; L.ow = p.out_w;
        L.first_char = first_char[i]; L.n_chars = count[i];
        L.resized = (p.resized_h != p.paste_h || p.resized_w != p.paste_w) ? 1 : 0;
        L.has_score = p.has_score ? 1 : 0;

        // the three dense output planes
        const long long area = (long long)p.out_h * p.out_w;
        VKX_REQUIRE(p.image_off >= 0 && (unsigned long long)(p.image_off + 3 * area) <= dst_bytes, "line image outside dst");
        VKX_REQUIRE(p.mask_off >= 0 && (unsigned long long)(p.mask_off + area) <= dst_bytes, "line mask outside dst");
        ranges.emplace_back(p.image_off, p.image_off + 3 * area);
        ranges.emplace_back(p.mask_off, p.mask_off + area);
        L.img = dst + p.image_off; L.msk = dst + p.mask_off; L.scr = nullptr;
        if (L.has_score) {
            VKX_REQUIRE(p.score_off >= 0 && p.score_off % 4 == 0 && (unsigned long long)(p.score_off + 4 * area) <= dst_bytes,
                        "line score map outside dst or not aligned to 4 bytes");
            ranges.emplace_back(p.score_off, p.score_off + 4 * area);
            L.scr = (float *)(dst + p.score_off);
        }

        int rc;
        if ((rc = planner.plan(L.r_u8, false, p.interpolation, p.paste_h, p.paste_w, p.resized_h, p.resized_w))) return rc;
        if ((rc = planner.plan(L.r_f32, true, p.interpolation, p.paste_h, p.paste_w, p.resized_h, p.resized_w))) return rc;

        // the clean-up of a trimmed char
        L.cleanup = p.cleanup ? 1 : 0;
        L.t_char = L.k_char = L.first_char;
        for (int k = 0; k < 4; k++) L.tb[k] = L.kb[k] = 0;
        L.r_t = L.r_k = vkd::PlannedResize{vkd::ResizePlan(), 0, 1, 1, 1, 1};
        if (L.cleanup) {
            VKX_REQUIRE(p.trimmed_char >= 0 && p.trimmed_char < count[i] && p.kept_char >= 0 && p.kept_char < count[i],
                        "clean-up char outside its line");
            for (int k = 0; k < 4; k++) {
                VKX_REQUIRE(p.trimmed_box[k] >= (k < 2 ? 0 : 1) && p.trimmed_box[k] <= kMaxSide, "trimmed char box outside 0 .. 32767");
                VKX_REQUIRE(p.kept_box[k] >= (k < 2 ? 0 : 1) && p.kept_box[k] <= kMaxSide, "kept char box outside 0 .. 32767");
                L.tb[k] = p.trimmed_box[k]; L.kb[k] = p.kept_box[k];
            }
            VKX_REQUIRE(p.kept_box[0] + p.kept_box[2] <= p.out_h && p.kept_box[1] + p.kept_box[3] <= p.out_w, "kept char box outside its line");
            L.t_char = L.first_char + p.trimmed_char; L.k_char = L.first_char + p.kept_char;
            const vkx_text_char &t = chars_host[L.t_char], &k = chars_host[L.k_char];
            if ((rc = planner.plan(L.r_t, false, p.interpolation, t.glyph_h, t.glyph_w, p.trimmed_box[2], p.trimmed_box[3]))) return rc;
            if (L.has_score && (rc = planner.plan(L.r_k, true, p.interpolation, k.glyph_h, k.glyph_w, p.kept_box[2], p.kept_box[3]))) return rc;
        }

        // the tiles of the two grids; the scratch planes of a resized line (offsets for now)
        const int dom_h = L.resized ? p.paste_h : p.out_h, dom_w = L.resized ? p.paste_w : p.out_w;
        paste_jobs[i] = TileJob{i, (int)paste_blocks};
        paste_blocks += (long long)((dom_w + 63) / 64) * ((dom_h + 3) / 4);
        L.s_img = L.s_msk = nullptr; L.s_scr = nullptr;
        if (L.resized) {
            resize_jobs.push_back(TileJob{i, (int)resize_blocks});
            resize_blocks += (long long)((p.out_w + 63) / 64) * ((p.out_h + 3) / 4);
            const long long pasted = (long long)p.paste_h * p.paste_w;
            L.s_scr = (float *)(uintptr_t)scratch_bytes;
            L.s_img = (uint8_t *)(uintptr_t)(scratch_bytes + 4 * pasted);
            L.s_msk = (uint8_t *)(uintptr_t)(scratch_bytes + 7 * pasted);
            scratch_bytes = (long long)vkx_align256((size_t)(scratch_bytes + 8 * pasted));
        }
        VKX_REQUIRE(paste_blocks < (1ll << 30) && resize_blocks < (1ll << 30) && scratch_bytes < (1ll << 40), "too many pixels for one call");
    }
    VKX_REQUIRE(!vkx_ranges_overlap(ranges), "line destinations overlap one another");

    for (int i = 0; i < n_chars; i++) {
        const vkx_text_char &p = chars_host[i];
        const vkx_text_line &lp = lines_host[p.line];
        VKX_REQUIRE(p.glyph_h >= 1 && p.glyph_w >= 1 && p.glyph_h <= kMaxSide && p.glyph_w <= kMaxSide, "glyph side outside 1 .. 32767");
        VKX_REQUIRE(p.up >= 0 && p.left >= 0 && p.up <= lp.paste_h - p.glyph_h && p.left <= lp.paste_w - p.glyph_w, "a char box outside its line");
        const size_t area = (size_t)p.glyph_h * p.glyph_w;
        VKX_REQUIRE(in_blob(p.image_off, area * (size_t)lp.channels), "glyph image outside the blob");
        VKX_REQUIRE(lp.has_score ? (p.score_off % 4 == 0 && in_blob(p.score_off, area * 4)) : p.score_off == -1,
                    "glyph score map outside the blob, not aligned to 4 bytes, or given to a line without one");
        VKX_REQUIRE(p.paste_off == -1 || (lp.channels == 3 && in_blob(p.paste_off, area * 3)), "glyph paste plane outside the blob, or given to a 1-channel glyph");
    }

    // one staged block: records, tile jobs, table blocks, the blob
    vkx_tables tab(ctx);
    const size_t lines_off = tab.add(sizeof(LineRec) * (size_t)n_lines);
    const size_t chars_off = tab.add(sizeof(CharRec) * (size_t)n_chars);
    const size_t pjobs_off = tab.add(sizeof(TileJob) * (size_t)n_lines);
    const size_t rjobs_off = tab.add(sizeof(TileJob) * std::max(resize_jobs.size(), (size_t)1));
    planner.layout([&](size_t bytes) { return tab.add(bytes); });
    const size_t lcd_off = tab.add(256);
    const size_t blob_off = tab.add(blob_bytes);

    int rc;
    if ((rc = tab.take())) return rc;
    planner.pack(tab.at<unsigned char>(0));          // (before the records are copied: packing completes the plans)
    fill_lcd_values(tab.at<uint8_t>(lcd_off));
    memcpy(tab.at<unsigned char>(blob_off), blob_host, blob_bytes);
    if ((rc = vkx_scratch_reserve(ctx, &ctx->text_tables, std::max(tab.bytes, (size_t)256 << 10)))) return rc;
    if ((rc = vkx_scratch_reserve(ctx, &ctx->text_planes, std::max((size_t)scratch_bytes, (size_t)256 << 10)))) return rc;
    const unsigned char *base = (const unsigned char *)ctx->text_tables.ptr;
    unsigned char *planes = (unsigned char *)ctx->text_planes.ptr;
    for (auto &L : lines)
        if (L.resized) {
            L.s_scr = (float *)(planes + (uintptr_t)L.s_scr);
            L.s_img = planes + (uintptr_t)L.s_img;
            L.s_msk = planes + (uintptr_t)L.s_msk;
        }
    for (int i = 0; i < n_chars; i++) {
        const vkx_text_char &p = chars_host[i];
        CharRec &g = chars[i];
        g.image = base + blob_off + p.image_off;
        g.score = p.score_off >= 0 ? (const float *)(base + blob_off + p.score_off) : nullptr;
        g.paste = p.paste_off >= 0 ? base + blob_off + p.paste_off : nullptr;
        g.gh = p.glyph_h; g.gw = p.glyph_w; g.up = p.up; g.left = p.left;
    }
    memcpy(tab.at<LineRec>(lines_off), lines.data(), sizeof(LineRec) * (size_t)n_lines);
    memcpy(tab.at<CharRec>(chars_off), chars.data(), sizeof(CharRec) * (size_t)n_chars);
    memcpy(tab.at<TileJob>(pjobs_off), paste_jobs.data(), sizeof(TileJob) * (size_t)n_lines);
    if (!resize_jobs.empty()) memcpy(tab.at<TileJob>(rjobs_off), resize_jobs.data(), sizeof(TileJob) * resize_jobs.size());
    if ((rc = tab.copy_to(ctx->text_tables.ptr))) return rc;
    const LineRec *d_lines = (const LineRec *)(base + lines_off);
    const CharRec *d_chars = (const CharRec *)(base + chars_off);
    {
        VKX_TIMED(ctx, "k_text_paste");
        k_text_paste<<<(unsigned)paste_blocks, 256, 0, ctx->stream>>>(d_lines, d_chars, (const TileJob *)(base + pjobs_off), n_lines, base,
                                                                               base + lcd_off);
    }
    VKX_LAUNCH_CHECK();
    {
        VKX_TIMED(ctx, "k_text_resize");
        k_text_resize<<<(unsigned)std::max(resize_blocks, 1ll), 256, 0, ctx->stream>>>(d_lines, d_chars, (const TileJob *)(base + rjobs_off),
                                                                                        (int)resize_jobs.size(), base);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
