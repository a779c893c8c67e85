// fill_text_line_to_seal_impression on gfx950 (reference: vkit/engine/seal_impression/text_line_slot_filler.py:28-205; the
// call PageAssemblerStep.run makes per seal, pipeline/text_detection/page_assembler.py:200).
//
// Per char the reference resizes the glyph's score map (or its mask) to the slot's aspect, lays it into a plane of the text
// line's height, rotates that plane (cv.warpAffine) into its slot on the ellipse and fills it into the seal's score map
// keeping the maximum; then the internal text line overwrites its box and the map is rescaled to alpha / max.  A seal has
// 20 - 60 chars of a few hundred pixels: composed from the single-plane operations that is three launches and a host round
// trip a char.  Here one call takes EVERY char of EVERY seal of a page, its records, tap tables and host glyph planes staged
// as one block (vkx_tables, one copy out of the ring), in three launches and without a synchronisation:
//   k_seal_planes   one workgroup column a char: the glyph resized into its char plane in context scratch (per pixel the
//                   functions of vkx_resize_pixel.h the kernels of resize.hip call, on the same table blocks); score maps clipped to [0, 1], masks as
//                   (resize((m > 0) * 255) > 0).  Also clears the per-seal maxima.
//   k_seal_gather   one lane a seal pixel: over the chars of its seal whose destination box covers it, the warp sample of
//                   the char plane (vkx_warp_affine_f32_dev's pixel), kept when the running value is smaller (`mat < value`
//                   of fill_np_array: a NaN and a -0.0 never replace anything, so the order does not matter).  Then the
//                   internal line's overwrite, the store, and ONE atomic a workgroup for the seal's maximum (a NaN wins).
//   k_seal_scale    map * float32(alpha) / max, two float32 roundings; an all-zero map gives 0 / 0 = NaN as numpy does.
// The planes are tens of kilobytes: the call is bound by launches and latency.
#include "vkx_internal.h"
#include "vkx_resize_pixel.h"
#include "vkx_warp.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace {

constexpr int kMaxChars = 4096, kMaxSeals = 256;
constexpr int kMaxSide = 32767;
constexpr int kCharGroups = 64;                 // at most this many workgroups stride over the pixels of one char plane
constexpr unsigned kNanKey = 0xffffffffu;

struct CharRec {
    const unsigned char *src;
    long long src_step;                         // bytes
    vkd::PlannedResize resize;                  // the glyph -> glyph_h x plane_w (M_COPY: the source has that shape); dw is the plane's width
    long long plane_off;                        // its plane in the plane scratch, floats
    int ph, glyph_up;                           // the plane is ph x resize.dw, the glyph in its rows from glyph_up
    int identity;                               // the rotation is a nop: the plane itself is filled
    int src_kind;                               // VKX_SEAL_SRC_F32 / _U8C1 / _U8C3
    double m[6];                                // CoordAffine's inverse matrix
    int rh, rw, seal, up, left;                 // the rotated plane and where it lands in its seal
};
static_assert(sizeof(CharRec) == 176, "k_seal_gather walks these records: no padding, the resize in front of what the gather reads");

struct SealRec {
    long long dst_off;                          // floats
    int h, w;
    float alpha;
    int first_char, n_chars;                    // its chars are consecutive in the table
    int first_block;                            // of the gather and scale grids
    const unsigned char *internal;
    long long internal_step;                    // bytes
    int internal_kind;                          // -1: none
    int iup, ileft, ih, iw;
};

struct Src {
    const unsigned char *p;
    long long step;
    int kind;
    __device__ __forceinline__ float f(int y, int x) const { return ((const float *)(p + (ptrdiff_t)y * step))[x]; }
    // (mask > 0) * 255 of Mask.to_resized_mask, the mask being any(image > 0) of CharGlyph.get_glyph_mask
    __device__ __forceinline__ int u(int y, int x) const
    {
        const unsigned char *r = p + (ptrdiff_t)y * step;
        if (kind == VKX_SEAL_SRC_U8C1) return r[x] ? 255 : 0;
        r += 3 * (ptrdiff_t)x;
        return (r[0] | r[1] | r[2]) ? 255 : 0;
    }
};

// grid: (max(chars, 1), groups); the workgroups of a char stride over the pixels of its plane.  A pixel of the resized glyph is the
// char's planned pixel of vkx_resize_pixel.h, read through Src; the source kind is the char's, so it is decided outside the loop.
__global__ void __launch_bounds__(256) k_seal_planes(const CharRec *__restrict__ recs, int n_chars, const unsigned char *__restrict__ tabs,
                                                     float *__restrict__ planes, unsigned *__restrict__ seal_max, int n_seals)
{
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < n_seals; i += 256) seal_max[i] = 0u;
    if ((int)blockIdx.x >= n_chars) return;
    const CharRec r = recs[blockIdx.x];
    const Src s{r.src, r.src_step, r.src_kind};
    const int n = r.ph * r.resize.dw;           // sides <= 32767: below 2^30
    float *plane = planes + r.plane_off;
    const auto fill = [&](auto glyph_pixel) {
        for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
            const int y = i / r.resize.dw, x = i - y * r.resize.dw, gy = y - r.glyph_up;
            plane[i] = (unsigned)gy < (unsigned)r.resize.dh ? glyph_pixel(gy, x) : 0.f;
        }
    };
    if (r.src_kind == VKX_SEAL_SRC_F32)         // a score map: np.clip(mat, 0, 1) of to_resized_score_map, unless it has the glyph's shape already
        fill([&](int dy, int dx) { return vkd::planned_pixel_f32(r.resize, tabs, dy, dx, [&](int y, int x) { return s.f(y, x); }); });
    else
        fill([&](int dy, int dx) {
            uint8_t vu;
            vkd::planned_pixel_u8<1>(r.resize, tabs, dy, dx, [&](int y, int x) { return s.u(y, x); }, &vu);
            return vu > 0 ? 1.f : 0.f;          // Mask.to_resized_mask's `> 0`, then mat.astype(np.float32)
        });
}

// float32 -> a key whose unsigned order is the order of the values; every NaN is the largest key (np.max returns NaN then)
__device__ __forceinline__ unsigned max_key(float v)
{
    if (v != v) return kNanKey;
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k)
{
    if (k == kNanKey) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the seal of a workgroup of the gather and scale grids, and the workgroup's 64 x 4 tile of it
__device__ __forceinline__ int seal_tile_pixel(const SealRec *seals, int n_seals, int &x, int &y)
{
    return vkd::box_tile_pixel<64, 4>(n_seals, [&](int i) { return seals[i].first_block; }, [&](int i) { return seals[i].w; }, x, y);
}

__global__ void __launch_bounds__(256) k_seal_gather(const CharRec *__restrict__ recs, const SealRec *__restrict__ seals, int n_seals,
                                                     const float *__restrict__ planes, float *__restrict__ dst,
                                                     unsigned *__restrict__ seal_max)
{
    __shared__ unsigned part[4];
    int x, y;
    const int si = seal_tile_pixel(seals, n_seals, x, y);
    const SealRec s = seals[si];
    unsigned key = 0u;                          // below every value's key
    if (x < s.w && y < s.h) {
        float v = 0.f;                          // ScoreMap.from_shape
        for (int c = s.first_char; c < s.first_char + s.n_chars; c++) {
            const CharRec &r = recs[c];
            const int ry = y - r.up, rx = x - r.left;
            if ((unsigned)ry >= (unsigned)r.rh || (unsigned)rx >= (unsigned)r.rw) continue;
            const float *plane = planes + r.plane_off;
            float q;
            if (r.identity) q = plane[(ptrdiff_t)ry * r.resize.dw + rx];
            else {
                vkd::CoordAffine coord;
#pragma unroll
                for (int i = 0; i < 6; i++) coord.m[i] = r.m[i];
                int X, Y;
                coord(rx, ry, X, Y);
                q = vkd::sample_f32(plane, r.ph, r.resize.dw, (ptrdiff_t)r.resize.dw, X, Y);
            }
            if (v < q) v = q;                   // fill_np_array(keep_max_value=True): np.putmask(mat, mat < value, value)
        }
        const int iy = y - s.iup, ix = x - s.ileft;
        if (s.internal_kind >= 0 && (unsigned)iy < (unsigned)s.ih && (unsigned)ix < (unsigned)s.iw) {
            const unsigned char *row = s.internal + (ptrdiff_t)iy * s.internal_step;
            v = s.internal_kind == VKX_SEAL_SRC_F32 ? ((const float *)row)[ix] : (float)row[ix];
        }
        dst[s.dst_off + (ptrdiff_t)y * s.w + x] = v;
        key = max_key(v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(seal_max + si, max(max(part[0], part[1]), max(part[2], part[3])));
}

__global__ void __launch_bounds__(256) k_seal_scale(const SealRec *__restrict__ seals, int n_seals, float *__restrict__ dst,
                                                    const unsigned *__restrict__ seal_max)
{
    int x, y;
    const int si = seal_tile_pixel(seals, n_seals, x, y);
    const SealRec s = seals[si];
    if (x >= s.w || y >= s.h) return;
    const float top = key_value(seal_max[si]);
    float *p = dst + s.dst_off + (ptrdiff_t)y * s.w + x;
    const float scaled = *p * s.alpha;
    *p = scaled / top;
}

bool is_u8(int kind) { return kind == VKX_SEAL_SRC_U8C1 || kind == VKX_SEAL_SRC_U8C3; }
size_t elem_row_bytes(int kind, int w) { return kind == VKX_SEAL_SRC_F32 ? (size_t)w * 4 : (kind == VKX_SEAL_SRC_U8C3 ? (size_t)w * 3 : (size_t)w); }

}  // namespace

VKX_EXPORT int vkx_seal_fill_dev(vkx_ctx *ctx, const vkx_seal_char *chars_host, int n_chars, const vkx_seal_rec *seals_host,
                                 int n_seals, const void *planes_host, size_t planes_host_bytes, float *dst, size_t dst_floats)
{
    VKX_REQUIRE(n_chars >= 0 && n_chars <= kMaxChars, "0 .. 4096 chars");
    VKX_REQUIRE(n_seals >= 1 && n_seals <= kMaxSeals, "1 .. 256 seals");
    VKX_REQUIRE(ctx && seals_host && dst && (chars_host || n_chars == 0), "NULL argument");
    VKX_REQUIRE(planes_host || planes_host_bytes == 0, "NULL host planes");
    VKX_REQUIRE(dst_floats <= ((size_t)1 << 40), "dst beyond 2^40 floats");
    const size_t dst_bytes = dst_floats * sizeof(float);

    // a source: a device plane, or (VKX_SEAL_SRC_HOST) a dense or stepped plane at a byte offset of planes_host
    auto check_source = [&](const void *src, int kind, long long step, int h, int w) -> int {
        const int base = kind & ~VKX_SEAL_SRC_HOST;
        VKX_REQUIRE(base == VKX_SEAL_SRC_F32 || base == VKX_SEAL_SRC_U8C1 || base == VKX_SEAL_SRC_U8C3, "unknown source kind");
        VKX_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "source side outside 1 .. 32767");
        const size_t row = elem_row_bytes(base, w);
        VKX_REQUIRE_PITCH(step, (ptrdiff_t)row, h);
        VKX_REQUIRE(base != VKX_SEAL_SRC_F32 || ((uintptr_t)src % 4 == 0 && (h <= 1 || step % 4 == 0)), "float32 source not aligned to 4 bytes");
        if (kind & VKX_SEAL_SRC_HOST) {
            const unsigned long long off = (unsigned long long)(uintptr_t)src;
            VKX_REQUIRE(off <= planes_host_bytes && (unsigned long long)(h - 1) * (unsigned long long)step + row <= planes_host_bytes - off,
                        "host source outside planes_host");
        } else {
            VKX_REQUIRE(src != nullptr, "NULL source");
            VKX_REQUIRE_DISJOINT(src, h, (ptrdiff_t)step, row, dst, 1, 0, dst_bytes);
        }
        return VKX_OK;
    };

    std::vector<std::pair<long long, long long>> ranges;
    std::vector<SealRec> seals(n_seals);
    int blocks = 0;
    for (int i = 0; i < n_seals; i++) {
        const vkx_seal_rec &p = seals_host[i];
        VKX_REQUIRE(p.h >= 1 && p.w >= 1 && p.h <= kMaxSide && p.w <= kMaxSide, "seal side outside 1 .. 32767");
        const long long area = (long long)p.h * p.w;
        VKX_REQUIRE(p.dst_off >= 0 && (unsigned long long)(p.dst_off + area) <= dst_floats, "seal destination outside dst");
        ranges.emplace_back(p.dst_off, p.dst_off + area);
        SealRec &s = seals[i];
        s.dst_off = p.dst_off; s.h = p.h; s.w = p.w; s.alpha = (float)p.alpha;
        s.first_char = 0; s.n_chars = 0;
        s.internal = nullptr; s.internal_step = 0; s.internal_kind = -1; s.iup = s.ileft = s.ih = s.iw = 0;
        if (p.internal_kind != VKX_SEAL_INTERNAL_NONE) {
            VKX_REQUIRE((p.internal_kind & ~VKX_SEAL_SRC_HOST) != VKX_SEAL_SRC_U8C3, "the internal text line is a float32 or a 1-channel uint8 plane");
            if (int rc = check_source(p.internal, p.internal_kind, p.internal_step, p.internal_h, p.internal_w)) return rc;
            VKX_REQUIRE(p.internal_up >= 0 && p.internal_left >= 0 && p.internal_up <= p.h - p.internal_h && p.internal_left <= p.w - p.internal_w,
                        "internal text line box outside its seal");
            s.internal = (const unsigned char *)p.internal; s.internal_step = p.internal_step; s.internal_kind = p.internal_kind;
            s.iup = p.internal_up; s.ileft = p.internal_left; s.ih = p.internal_h; s.iw = p.internal_w;
        }
        s.first_block = blocks;
        const long long tiles = (long long)((p.w + 63) / 64) * ((p.h + 3) / 4);
        VKX_REQUIRE(blocks + tiles < (1ll << 30), "too many pixels for one call");
        blocks += (int)tiles;
    }
    VKX_REQUIRE(!vkx_ranges_overlap(ranges), "seal destinations overlap one another");

    // chars: checked, planned, and laid out behind the records in one staged block
    std::vector<CharRec> chars(n_chars);
    vkd::ResizePlanner planner(__func__);
    vkx_tables tab(ctx);
    const size_t chars_off = tab.add(sizeof(CharRec) * (size_t)std::max(n_chars, 1));
    const size_t seals_off = tab.add(sizeof(SealRec) * (size_t)n_seals);
    long long plane_floats = 0;
    int groups = 1;
    for (int i = 0; i < n_chars; i++) {
        const vkx_seal_char &p = chars_host[i];
        CharRec &r = chars[i];
        if (int rc = check_source(p.src, p.src_kind, p.src_step, p.src_h, p.src_w)) return rc;
        VKX_REQUIRE(p.plane_h >= 1 && p.plane_w >= 1 && p.plane_h <= kMaxSide && p.plane_w <= kMaxSide, "char plane side outside 1 .. 32767");
        VKX_REQUIRE(p.glyph_h >= 1 && p.glyph_up >= 0 && p.glyph_up <= p.plane_h - p.glyph_h, "glyph rows outside the char plane");
        VKX_REQUIRE(p.rot_h >= 1 && p.rot_w >= 1 && p.rot_h <= kMaxSide && p.rot_w <= kMaxSide, "rotated plane side outside 1 .. 32767");
        VKX_REQUIRE(p.seal >= 0 && p.seal < n_seals, "seal index outside the table");
        VKX_REQUIRE(i == 0 || p.seal >= chars_host[i - 1].seal, "chars not grouped by ascending seal");
        const vkx_seal_rec &sp = seals_host[p.seal];
        VKX_REQUIRE(p.dst_up >= 0 && p.dst_left >= 0 && p.dst_up <= sp.h - p.rot_h && p.dst_left <= sp.w - p.rot_w,
                    "a char destination box outside its seal");
        VKX_REQUIRE(!p.identity || (p.rot_h == p.plane_h && p.rot_w == p.plane_w), "an identity rotation keeps the plane's size");
        VKX_REQUIRE(vkd::ResizePlanner::known_interpolation(p.interpolation), "unknown interpolation code");
        const bool f32 = (p.src_kind & ~VKX_SEAL_SRC_HOST) == VKX_SEAL_SRC_F32;
        r.src = (const unsigned char *)p.src; r.src_step = p.src_step; r.src_kind = p.src_kind;
        r.ph = p.plane_h; r.glyph_up = p.glyph_up;
        if (int rc = planner.plan(r.resize, f32, p.interpolation, p.src_h, p.src_w, p.glyph_h, p.plane_w)) return rc;
        r.identity = p.identity ? 1 : 0;
        double forward[6];
        for (int k = 0; k < 6; k++) forward[k] = (double)p.m[k];
        const vkd::CoordAffine c = vkd::make_affine(forward);
        for (int k = 0; k < 6; k++) r.m[k] = c.m[k];
        r.rh = p.rot_h; r.rw = p.rot_w; r.seal = p.seal; r.up = p.dst_up; r.left = p.dst_left;
        r.plane_off = plane_floats;
        plane_floats += (long long)p.plane_h * p.plane_w;
        groups = std::max(groups, std::min(kCharGroups, (p.plane_h * p.plane_w + 255) / 256));
        SealRec &s = seals[p.seal];
        if (s.n_chars++ == 0) s.first_char = i;
    }
    planner.layout([&](size_t bytes) { return tab.add(bytes); });
    const size_t host_off = planes_host_bytes ? tab.add(planes_host_bytes) : 0;

    int rc;
    if ((rc = tab.take())) return rc;
    planner.pack(tab.at<unsigned char>(0));          // (before the records are copied: packing completes the plans)
    if (planes_host_bytes) memcpy(tab.at<unsigned char>(host_off), planes_host, planes_host_bytes);
    // the staged block lands in seal_tables: host sources are addressed there
    if ((rc = vkx_scratch_reserve(ctx, &ctx->seal_tables, std::max(tab.bytes, (size_t)64 << 10)))) return rc;
    const unsigned char *base = (const unsigned char *)ctx->seal_tables.ptr;
    for (int i = 0; i < n_chars; i++) {
        CharRec &r = chars[i];
        if (r.src_kind & VKX_SEAL_SRC_HOST) { r.src = base + host_off + (uintptr_t)r.src; r.src_kind &= ~VKX_SEAL_SRC_HOST; }
    }
    for (auto &s : seals)
        if (s.internal_kind >= 0 && (s.internal_kind & VKX_SEAL_SRC_HOST)) {
            s.internal = base + host_off + (uintptr_t)s.internal; s.internal_kind &= ~VKX_SEAL_SRC_HOST;
        }
    if (n_chars) memcpy(tab.at<CharRec>(chars_off), chars.data(), sizeof(CharRec) * (size_t)n_chars);
    memcpy(tab.at<SealRec>(seals_off), seals.data(), sizeof(SealRec) * (size_t)n_seals);
    const size_t max_off = vkx_align256(sizeof(float) * (size_t)std::max(plane_floats, 1ll));
    if ((rc = vkx_scratch_reserve(ctx, &ctx->seal_planes, std::max(max_off + sizeof(unsigned) * kMaxSeals, (size_t)256 << 10)))) return rc;
    if ((rc = tab.copy_to(ctx->seal_tables.ptr))) return rc;
    const CharRec *d_chars = (const CharRec *)(base + chars_off);
    const SealRec *d_seals = (const SealRec *)(base + seals_off);
    float *planes = (float *)ctx->seal_planes.ptr;
    unsigned *seal_max = (unsigned *)((unsigned char *)ctx->seal_planes.ptr + max_off);
    {
        VKX_TIMED(ctx, "k_seal_planes");
        k_seal_planes<<<dim3(std::max(n_chars, 1), groups), 256, 0, ctx->stream>>>(d_chars, n_chars, base, planes, seal_max, n_seals);
    }
    VKX_LAUNCH_CHECK();
    {
        VKX_TIMED(ctx, "k_seal_gather");
        k_seal_gather<<<blocks, 256, 0, ctx->stream>>>(d_chars, d_seals, n_seals, planes, dst, seal_max);
    }
    VKX_LAUNCH_CHECK();
    {
        VKX_TIMED(ctx, "k_seal_scale");
        k_seal_scale<<<blocks, 256, 0, ctx->stream>>>(d_seals, n_seals, dst, seal_max);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
