// PageCroppingStep / Cropper on gfx950 (reference: pipeline/text_detection/page_cropping.py:87-290, mechanism/cropper.py).
//
// The step's host loop draws crop windows, crops seven planes per window, counts label pixels to accept or reject it
// and shrinks the five label planes of an accepted crop with cv.resize(INTER_AREA).  Here the windows are worked out on
// the host (vkit_amd/pipeline/text_detection/page_cropping.py) and the pixels take two launches:
//   k_crop_count   every candidate window's two counts (+ the page's nonzero pixels) as per-workgroup partial sums;
//   k_crop_planes  every plane of every accepted crop: the window copied, the rest filled, and for a core-only plane the
//                  integer-factor INTER_AREA shrink computed from the same reads (vkd::area_fast_* of vkx_resize_pixel.h, shared with resize.hip).
// Both are gathers bound by HBM reads of the page windows; the tables (windows, planes) travel as one small copy each.
#include "vkx_internal.h"
#include "vkx_resize_pixel.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int kCountThreads = 256;

__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    unsigned long long total = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kCountThreads / 64; i++) total += lds[i];
    __syncthreads();
    return total;
}

// grid (n_parts, 1 + n_windows): item 0 counts the page, item 1 + i window i; part p of an item takes every n_parts-th
// run of 256 pixels.
__global__ void __launch_bounds__(kCountThreads) k_crop_count(const uint8_t *__restrict__ image, int h, int w, int cn,
                                                              const uint8_t *__restrict__ active, const uint8_t *__restrict__ chars,
                                                              int core, int pad, const vkx_crop_window *__restrict__ windows,
                                                              int n_parts, long long *__restrict__ partials)
{
    __shared__ unsigned long long lds[kCountThreads / 64];
    const int item = blockIdx.y, part = blockIdx.x;
    const size_t step = (size_t)n_parts * kCountThreads;
    unsigned long long a = 0, b = 0;
    if (item == 0) {
        if (image) {
            const size_t n = (size_t)h * w;
            for (size_t i = (size_t)part * kCountThreads + threadIdx.x; i < n; i += step) {
                const uint8_t *p = image + i * cn;
                int any = 0;
                for (int c = 0; c < cn; c++) any |= p[c];
                a += any != 0;
            }
        }
    } else {
        const vkx_crop_window win = windows[item - 1];
        // the core in page coordinates (it may reach past the page: padding counts nothing)
        const int cu = win.up + pad - win.target_up, cl = win.left + pad - win.target_left;
        const size_t n = (size_t)win.height * win.width;
        for (size_t i = (size_t)part * kCountThreads + threadIdx.x; i < n; i += step) {
            const int y = win.up + (int)(i / win.width), x = win.left + (int)(i % win.width);
            const size_t at = (size_t)y * w + x;
            b += active[at] != 0;
            if (y >= cu && y < cu + core && x >= cl && x < cl + core) a += chars[at] != 0;
        }
    }
    a = block_sum(a, lds);
    b = block_sum(b, lds);
    if (threadIdx.x == 0) {
        long long *out = partials + ((size_t)item * n_parts + part) * 2;
        out[0] = (long long)a;
        out[1] = (long long)b;
    }
}

// grid (crop / 64, crop / 4, n_planes).  A full-crop plane: one lane per crop pixel.  A core-only plane: one lane per
// f x f cell of the core (f = factor, 1 without a shrink), which copies the cell and writes its shrunk sample.
__global__ void __launch_bounds__(256) k_crop_planes(int h, int w, int core, int pad, int factor,
                                                     const vkx_crop_window *__restrict__ windows,
                                                     const vkx_crop_plane *__restrict__ planes)
{
    const vkx_crop_plane P = planes[blockIdx.z];
    const vkx_crop_window win = windows[P.window];
    const int crop = core + 2 * pad;
    const int lx = blockIdx.x * 64 + (threadIdx.x & 63), ly = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int cn = P.cn;
    // source offset (in pixels) of crop pixel (ty, tx), or -1 in the padding
    auto src_index = [&](int ty, int tx) -> ptrdiff_t {
        const int sy = ty - win.target_up, sx = tx - win.target_left;
        if (sy < 0 || sy >= win.height || sx < 0 || sx >= win.width) return -1;
        return (ptrdiff_t)(win.up + sy) * w + (win.left + sx);
    };
    if (!P.core_only) {
        if (lx >= crop || ly >= crop) return;
        const ptrdiff_t s = src_index(ly, lx);
        const ptrdiff_t d = (ptrdiff_t)ly * crop + lx;
        if (P.is_f32) {
            ((float *)P.dst)[d] = s < 0 ? 0.f : ((const float *)P.src)[s];
        } else {
            const uint8_t *src = (const uint8_t *)P.src + s * cn;
            uint8_t *dst = (uint8_t *)P.dst + d * cn;
            for (int c = 0; c < cn; c++) dst[c] = s < 0 ? (uint8_t)P.fill : src[c];
        }
        return;
    }
    const int f = (factor && P.dst_down) ? factor : 1;
    const int cells = core / f;
    if (lx >= cells || ly >= cells) return;
    const int cy0 = ly * f, cx0 = lx * f;     // the cell in core coordinates
    const ptrdiff_t down = (ptrdiff_t)ly * cells + lx;
    if (P.is_f32) {
        const float *src = (const float *)P.src;
        float *dst = (float *)P.dst;
        // visits every cell sample once: copies it, hands it to the shrink
        auto at = [&](int y, int x) -> float {
            const ptrdiff_t s = src_index(pad + cy0 + y, pad + cx0 + x);
            const float v = s < 0 ? 0.f : src[s];
            dst[(ptrdiff_t)(cy0 + y) * core + cx0 + x] = v;
            return v;
        };
        if (f == 1) {
            at(0, 0);
            return;
        }
        float v = vkd::area_fast_f32(at, f, f);
        if (P.clip) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        ((float *)P.dst_down)[down] = v;
    } else {
        const uint8_t *src = (const uint8_t *)P.src;
        uint8_t *dst = (uint8_t *)P.dst;
        for (int c = 0; c < cn; c++) {
            auto at = [&](int y, int x) -> int {
                const ptrdiff_t s = src_index(pad + cy0 + y, pad + cx0 + x);
                const uint8_t v = s < 0 ? (uint8_t)P.fill : src[s * cn + c];
                dst[((ptrdiff_t)(cy0 + y) * core + cx0 + x) * cn + c] = v;
                return P.is_mask ? (v ? 255 : 0) : v;
            };
            if (f == 1) {
                at(0, 0);
                continue;
            }
            const uint8_t r = vkd::area_fast_u8(at, f, f);
            ((uint8_t *)P.dst_down)[down * cn + c] = P.is_mask ? (uint8_t)(r > 0) : r;
        }
    }
}

// windows inside the page and inside the crop
int check_windows(const vkx_crop_window *windows, int n, int h, int w, int crop)
{
    for (int i = 0; i < n; i++) {
        const vkx_crop_window &v = windows[i];
        VKX_REQUIRE(v.height >= 1 && v.width >= 1, "empty crop window");
        VKX_REQUIRE(v.up >= 0 && v.left >= 0 && (long long)v.up + v.height <= h && (long long)v.left + v.width <= w,
                    "crop window outside the page");
        VKX_REQUIRE(v.target_up >= 0 && v.target_left >= 0 && (long long)v.target_up + v.height <= crop &&
                        (long long)v.target_left + v.width <= crop,
                    "crop window outside the crop");
    }
    return VKX_OK;
}

bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return vkx_planes_overlap(a, 1, 0, a_bytes, b, 1, 0, b_bytes);
}

}  // namespace

VKX_EXPORT int vkx_crop_count_dev(vkx_ctx *ctx, const uint8_t *image, int h, int w, int cn, const uint8_t *active_mask,
                                  const uint8_t *char_mask, int core_size, int pad_size, const vkx_crop_window *windows_host,
                                  int n_windows, int n_parts, int64_t *partials)
{
    VKX_REQUIRE(ctx && active_mask && char_mask && partials && (windows_host || n_windows == 0), "NULL argument");
    VKX_REQUIRE(h >= 1 && w >= 1, "bad page shape");
    VKX_REQUIRE(cn == 1 || cn == 3 || cn == 4, "1, 3 or 4 channels");
    VKX_REQUIRE(core_size >= 1 && pad_size >= 0, "bad core / pad size");
    VKX_REQUIRE(n_windows >= 0 && n_windows < 65535, "0 .. 65534 windows");
    VKX_REQUIRE(n_parts >= 1 && n_parts <= 4096, "1 .. 4096 parts");
    int rc = check_windows(windows_host, n_windows, h, w, core_size + 2 * pad_size);
    if (rc) return rc;
    const size_t page = (size_t)h * w, out_bytes = sizeof(int64_t) * 2 * (size_t)n_parts * (1 + n_windows);
    for (const void *src : {(const void *)active_mask, (const void *)char_mask})
        VKX_REQUIRE(!ranges_overlap(src, page, partials, out_bytes), "source and destination overlap");
    if (image) VKX_REQUIRE(!ranges_overlap(image, page * cn, partials, out_bytes), "source and destination overlap");
    const vkx_crop_window *windows = nullptr;
    if (n_windows) {
        vkx_tables tab(ctx);
        if ((rc = tab.take(sizeof(vkx_crop_window) * n_windows))) return rc;
        memcpy(tab.host, windows_host, tab.bytes);
        if ((rc = tab.copy_to(&ctx->crop_windows, (size_t)64 << 10))) return rc;   // grows (and syncs) rarely
        windows = (const vkx_crop_window *)ctx->crop_windows.ptr;
    }
    dim3 grid(n_parts, 1 + n_windows);
    {
        VKX_TIMED(ctx, "k_crop_count");
        k_crop_count<<<grid, kCountThreads, 0, ctx->stream>>>(image, h, w, cn, active_mask, char_mask, core_size, pad_size, windows,
                                                              n_parts, (long long *)partials);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}

VKX_EXPORT int vkx_crop_planes_dev(vkx_ctx *ctx, int h, int w, int core_size, int pad_size, int factor, const vkx_crop_window *windows_host,
                                   int n_windows, const vkx_crop_plane *planes_host, int n_planes)
{
    VKX_REQUIRE(ctx && (windows_host || n_windows == 0) && (planes_host || n_planes == 0), "NULL argument");
    VKX_REQUIRE(h >= 1 && w >= 1, "bad page shape");
    VKX_REQUIRE(core_size >= 1 && pad_size >= 0, "bad core / pad size");
    VKX_REQUIRE(n_windows >= 0 && n_planes >= 0 && n_planes < 65535, "0 .. 65534 planes");
    VKX_REQUIRE(factor >= 0 && (factor == 0 || (core_size % factor == 0 && pad_size % factor == 0)),
                "the shrink factor divides the core and the pad");
    const int crop = core_size + 2 * pad_size;
    int rc = check_windows(windows_host, n_windows, h, w, crop);
    if (rc) return rc;
    // every destination against every source plane (the distinct ones: a step hands the same seven to every crop)
    std::vector<std::pair<const void *, size_t>> sources;
    for (int i = 0; i < n_planes; i++) {
        const vkx_crop_plane &p = planes_host[i];
        VKX_REQUIRE(p.src && p.dst, "NULL plane");
        VKX_REQUIRE(p.window >= 0 && p.window < n_windows, "window index out of range");
        VKX_REQUIRE(p.is_f32 == 0 || p.is_f32 == 1, "is_f32 is 0 or 1");
        VKX_REQUIRE(p.is_f32 ? p.cn == 1 : (p.cn == 1 || p.cn == 3 || p.cn == 4), "1, 3 or 4 channels (float32: 1)");
        VKX_REQUIRE(p.is_f32 ? p.fill == 0 : (p.fill >= 0 && p.fill <= 255), "fill 0 .. 255 (float32: 0)");
        VKX_REQUIRE(!p.dst_down || (p.core_only && factor), "a shrunk plane is core-only and needs a factor");
        const size_t esz = p.is_f32 ? 4 : 1, src_bytes = (size_t)h * w * p.cn * esz;
        bool seen = false;
        for (auto &s : sources) seen = seen || (s.first == p.src && s.second == src_bytes);
        if (!seen) sources.push_back({p.src, src_bytes});
    }
    for (int i = 0; i < n_planes; i++) {
        const vkx_crop_plane &p = planes_host[i];
        const size_t esz = p.is_f32 ? 4 : 1, side = p.core_only ? core_size : crop;
        const size_t dst_bytes = side * side * p.cn * esz;
        const size_t down_bytes = p.dst_down ? (size_t)(core_size / factor) * (core_size / factor) * p.cn * esz : 0;
        for (auto &s : sources) {
            VKX_REQUIRE(!ranges_overlap(s.first, s.second, p.dst, dst_bytes), "source and destination overlap");
            VKX_REQUIRE(!p.dst_down || !ranges_overlap(s.first, s.second, p.dst_down, down_bytes), "source and destination overlap");
        }
    }
    if (n_planes == 0) return VKX_OK;
    // the two tables keep a slot each (the count pass leaves its windows in theirs), so each travels as a copy of its own
    vkx_tables wins(ctx), planes(ctx);
    if ((rc = wins.take(sizeof(vkx_crop_window) * n_windows)) || (rc = planes.take(sizeof(vkx_crop_plane) * n_planes))) return rc;
    memcpy(wins.host, windows_host, wins.bytes);
    memcpy(planes.host, planes_host, planes.bytes);
    if ((rc = wins.copy_to(&ctx->crop_windows, (size_t)64 << 10)) || (rc = planes.copy_to(&ctx->crop_planes, (size_t)64 << 10))) return rc;
    dim3 grid(vkx_blocks(crop, 64), vkx_blocks(crop, 4), n_planes);
    {
        VKX_TIMED(ctx, "k_crop_planes");
        k_crop_planes<<<grid, 256, 0, ctx->stream>>>(h, w, core_size, pad_size, factor, (const vkx_crop_window *)ctx->crop_windows.ptr,
                                                     (const vkx_crop_plane *)ctx->crop_planes.ptr);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
