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
#include <memory>
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
    int src_kind;                               // VKX_SEAL_SRC_F32 / _U8C1 / _U8C3
    int sh, sw, gh;                             // the glyph is resized to gh x pw
    vkd::ResizePlan plan;                       // (M_COPY: the source has the glyph's shape)
    long long tab_off;                          // the char's table block, bytes from the start of the staged block
    long long plane_off;                        // its plane in the plane scratch, floats
    int ph, pw, glyph_up;
    int identity;                               // the rotation is a nop: the plane itself is filled
    double m[6];                                // CoordAffine's inverse matrix
    int rh, rw, seal, up, left;                 // the rotated plane and where it lands in its seal
};

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

// CUBIC / LANCZOS4 of a glyph: the tap pixel on the char's tap block
template <int KS>
__device__ __forceinline__ void glyph_taps(const Src &s, bool f32, const unsigned char *tab, int sh, int sw, int dh, int dw, int dy, int dx,
                                           float *vf, uint8_t *vu)
{
    if (f32) {
        const vkd::TapView<float> t(tab, KS, dh, dw);
        *vf = vkd::taps_pixel_f32<KS>([&](int y, int x) { return s.f(y, x); }, sh, sw, t.xofs[dx], t.yofs[dy], t.xcoef + KS * dx, t.ycoef + KS * dy);
    } else {
        const vkd::TapView<short> t(tab, KS, dh, dw);
        vkd::taps_pixel_u8<1, KS>([&](int y, int x) { return s.u(y, x); }, sh, sw, t.xofs[dx], t.yofs[dy], t.xcoef + KS * dx, t.ycoef + KS * dy, vu);
    }
}

// One pixel of the resized glyph as the char plane holds it: the pixel of vkx_resize_pixel.h the char's plan names, read through Src.
__device__ float glyph_pixel(const CharRec &r, const unsigned char *tabs, int dy, int dx)
{
    const Src s{r.src, r.src_step, r.src_kind};
    const bool f32 = r.src_kind == VKX_SEAL_SRC_F32;
    const int sh = r.sh, sw = r.sw, dh = r.gh, dw = r.pw;
    const int *p = r.plan.p;
    const unsigned char *tab = tabs + r.tab_off;
    float vf = 0.f;
    uint8_t vu = 0;
    switch (r.plan.mode) {
    case vkd::M_COPY:
        if (f32) return s.f(dy, dx);            // (a matching score map is filled as it is: no clip)
        vu = (uint8_t)s.u(dy, dx);
        break;
    case vkd::M_NEAREST_EXACT: {
        const int sx = vkd::nearest_exact_index(dx, p[0], p[1], sw), sy = vkd::nearest_exact_index(dy, p[2], p[3], sh);
        if (f32) vf = s.f(sy, sx); else vu = (uint8_t)s.u(sy, sx);
        break;
    }
    case vkd::M_LINEAR_F32:
        vf = vkd::linear_pixel_f32([&](int y, int x) { return s.f(y, x); }, sh, sw, dy, dx, r.plan.scale_x, r.plan.scale_y);
        break;
    case vkd::M_LINEAR_EXACT_U8:
        vkd::linear_exact_pixel_u8<1>([&](int y, int below, int x, int) { return s.u(y + below, x); }, vkd::LinearExactView::of(tab, dh, dw), p, dh, dw, dy, dx, &vu);
        break;
    case vkd::M_HALF_U8: vkd::half_pixel_u8<1>([&](int y, int x, int) { return s.u(2 * dy + y, 2 * dx + x); }, &vu); break;
    case vkd::M_TAPS:
        if (r.plan.ks == 4) glyph_taps<4>(s, f32, tab, sh, sw, dh, dw, dy, dx, &vf, &vu);
        else glyph_taps<8>(s, f32, tab, sh, sw, dh, dw, dy, dx, &vf, &vu);
        break;
    case vkd::M_AREA_FAST:
        if (f32) vf = vkd::area_fast_f32([&](int y, int x) { return s.f(dy * p[1] + y, dx * p[0] + x); }, p[0], p[1]);
        else vu = vkd::area_fast_u8([&](int y, int x) { return s.u(dy * p[1] + y, dx * p[0] + x); }, p[0], p[1]);
        break;
    default:                                    // M_AREA
        if (f32) vkd::area_pixel<1, true>([&](int y, int x, int) { return s.f(y, x); }, vkd::AreaView(tab, dh, dw), dy, dx, &vf);
        else vkd::area_pixel<1, false>([&](int y, int x, int) { return (float)s.u(y, x); }, vkd::AreaView(tab, dh, dw), dy, dx, &vu);
        break;
    }
    if (!f32) return vu > 0 ? 1.f : 0.f;        // Mask.to_resized_mask's `> 0`, then mat.astype(np.float32)
    return vf < 0.f ? 0.f : (vf > 1.f ? 1.f : vf);   // np.clip(mat, 0, 1) of to_resized_score_map; a NaN stays
}

// grid: (max(chars, 1), groups); the workgroups of a char stride over the pixels of its plane
__global__ void __launch_bounds__(256) k_seal_planes(const CharRec *__restrict__ recs, int n_chars, const unsigned char *__restrict__ tabs,
                                                     float *__restrict__ planes, unsigned *__restrict__ seal_max, int n_seals)
{
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < n_seals; i += 256) seal_max[i] = 0u;
    if ((int)blockIdx.x >= n_chars) return;
    const CharRec r = recs[blockIdx.x];
    const int n = r.ph * r.pw;                  // sides <= 32767: below 2^30
    float *plane = planes + r.plane_off;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
        const int y = i / r.pw, x = i - y * r.pw, gy = y - r.glyph_up;
        plane[i] = (unsigned)gy < (unsigned)r.gh ? glyph_pixel(r, tabs, gy, x) : 0.f;
    }
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
__device__ __forceinline__ int seal_of_block(const SealRec *seals, int n_seals, int block)
{
    return vkd::last_at_most(n_seals, block, [&](int i) { return seals[i].first_block; });
}

__global__ void __launch_bounds__(256) k_seal_gather(const CharRec *__restrict__ recs, const SealRec *__restrict__ seals, int n_seals,
                                                     const float *__restrict__ planes, float *__restrict__ dst,
                                                     unsigned *__restrict__ seal_max)
{
    __shared__ unsigned part[4];
    const int si = seal_of_block(seals, n_seals, blockIdx.x);
    const SealRec s = seals[si];
    const int tiles_x = (s.w + 63) >> 6, t = blockIdx.x - s.first_block;
    const int x = (t % tiles_x) * 64 + (threadIdx.x & 63), y = (t / tiles_x) * 4 + (threadIdx.x >> 6);
    unsigned key = 0u;                          // below every value's key
    if (x < s.w && y < s.h) {
        float v = 0.f;                          // ScoreMap.from_shape
        for (int c = s.first_char; c < s.first_char + s.n_chars; c++) {
            const CharRec &r = recs[c];
            const int ry = y - r.up, rx = x - r.left;
            if ((unsigned)ry >= (unsigned)r.rh || (unsigned)rx >= (unsigned)r.rw) continue;
            const float *plane = planes + r.plane_off;
            float q;
            if (r.identity) q = plane[(ptrdiff_t)ry * r.pw + rx];
            else {
                vkd::CoordAffine coord;
#pragma unroll
                for (int i = 0; i < 6; i++) coord.m[i] = r.m[i];
                int X, Y;
                coord(rx, ry, X, Y);
                q = vkd::sample_f32(plane, r.ph, r.pw, (ptrdiff_t)r.pw, X, Y);
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
    const int si = seal_of_block(seals, n_seals, blockIdx.x);
    const SealRec s = seals[si];
    const int tiles_x = (s.w + 63) >> 6, t = blockIdx.x - s.first_block;
    const int x = (t % tiles_x) * 64 + (threadIdx.x & 63), y = (t / tiles_x) * 4 + (threadIdx.x >> 6);
    if (x >= s.w || y >= s.h) return;
    const float top = key_value(seal_max[si]);
    float *p = dst + s.dst_off + (ptrdiff_t)y * s.w + x;
    const float scaled = *p * s.alpha;
    *p = scaled / top;
}

bool is_u8(int kind) { return kind == VKX_SEAL_SRC_U8C1 || kind == VKX_SEAL_SRC_U8C3; }
size_t elem_row_bytes(int kind, int w) { return kind == VKX_SEAL_SRC_F32 ? (size_t)w * 4 : (kind == VKX_SEAL_SRC_U8C3 ? (size_t)w * 3 : (size_t)w); }

bool known_interpolation(int c)
{
    return c == VKX_INTER_CUBIC || c == VKX_INTER_AREA || c == VKX_INTER_LANCZOS4 || c == VKX_INTER_LINEAR_EXACT || c == VKX_INTER_NEAREST_EXACT;
}

// the bytes of a char's table block (none: 0); given an address, the block is written there (and a LINEAR_EXACT plan gets its ranges)
size_t pack_tables(CharRec &r, bool f32, const vkd::AreaTabs *area, unsigned char *out)
{
    switch (r.plan.mode) {
    case vkd::M_TAPS: return vkd::pack_taps(r.plan.ks, f32, r.sh, r.sw, r.gh, r.pw, out);
    case vkd::M_LINEAR_EXACT_U8: return vkd::pack_linear_exact(r.sh, r.sw, r.gh, r.pw, out, r.plan.p);
    case vkd::M_AREA: return area->pack(out);
    default: return 0;
    }
}

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
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++) VKX_REQUIRE(ranges[i].first >= ranges[i - 1].second, "seal destinations overlap one another");

    // chars: checked, planned, and laid out behind the records in one staged block
    std::vector<CharRec> chars(n_chars);
    std::vector<std::unique_ptr<vkd::AreaTabs>> area(n_chars);   // of the chars whose plan is M_AREA
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
        VKX_REQUIRE(known_interpolation(p.interpolation), "unknown interpolation code");
        const bool f32 = (p.src_kind & ~VKX_SEAL_SRC_HOST) == VKX_SEAL_SRC_F32;
        r.src = (const unsigned char *)p.src; r.src_step = p.src_step; r.src_kind = p.src_kind;
        r.sh = p.src_h; r.sw = p.src_w; r.gh = p.glyph_h;
        r.ph = p.plane_h; r.pw = p.plane_w; r.glyph_up = p.glyph_up;
        r.tab_off = 0;
        r.plan = vkd::ResizePlan();
        if (p.src_h != p.glyph_h || p.src_w != p.plane_w) {
            r.plan = vkd::plan_resize(f32, p.interpolation, p.src_h, p.src_w, p.glyph_h, p.plane_w);
            VKX_REQUIRE(!r.plan.refused(), "INTER_AREA is for shrinking only");
            if (r.plan.mode == vkd::M_AREA) area[i].reset(new vkd::AreaTabs(p.src_h, p.src_w, p.glyph_h, p.plane_w, r.plan.scale_x, r.plan.scale_y));
            if (const size_t bytes = pack_tables(r, f32, area[i].get(), nullptr)) r.tab_off = (long long)tab.add(bytes);
        }
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
    const size_t host_off = planes_host_bytes ? tab.add(planes_host_bytes) : 0;

    int rc;
    if ((rc = tab.take())) return rc;
    for (int i = 0; i < n_chars; i++) {
        CharRec &r = chars[i];
        if (r.tab_off) pack_tables(r, (r.src_kind & ~VKX_SEAL_SRC_HOST) == VKX_SEAL_SRC_F32, area[i].get(), tab.at<unsigned char>((size_t)r.tab_off));
    }
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
