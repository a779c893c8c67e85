// Host-pointer entry points: each names the caller's numpy planes and the *_dev implementation that runs on their staged copies
// (vkx_host_stage.h: to ctx scratch, the call on the ctx stream, the results back, synchronised).  Nothing here computes pixels.
#include "vkx_host_stage.h"

VKX_EXPORT int vkx_remap_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                            const float *map_x, const float *map_y, ptrdiff_t map_stride_el, uint8_t *dst, int dh,
                            int dw, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && map_x && map_y && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh >= 0 && dw >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, cn, src_stride);
    auto mx = vkx_in(map_x, dh, dw, 1, map_stride_el), my = vkx_in(map_y, dh, dw, 1, map_stride_el);
    auto d = vkx_out(dst, dh, dw, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &mx, &my, &d}, [&] {
        return vkx_remap_u8_dev(ctx, s.dev(), sh, sw, cn, s.pitch, mx.dev(), my.dev(), mx.pitch, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_remap_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                             const float *map_x, const float *map_y, ptrdiff_t map_stride_el, float *dst, int dh, int dw,
                             ptrdiff_t dst_stride_el)
{
    VKX_REQUIRE(ctx && src && map_x && map_y && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh >= 0 && dw >= 0, "bad shape");
    auto s = vkx_in(src, sh, sw, 1, src_stride_el);
    auto mx = vkx_in(map_x, dh, dw, 1, map_stride_el), my = vkx_in(map_y, dh, dw, 1, map_stride_el);
    auto d = vkx_out(dst, dh, dw, 1, dst_stride_el);
    return vkx_host_run(ctx, {&s, &mx, &my, &d}, [&] {
        return vkx_remap_f32_dev(ctx, s.dev(), sh, sw, s.pitch, mx.dev(), my.dev(), mx.pitch, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_warp_affine_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                                  const double M[6], uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && M && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh >= 0 && dw >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, cn, src_stride), d = vkx_out(dst, dh, dw, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_warp_affine_u8_dev(ctx, s.dev(), sh, sw, cn, s.pitch, M, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_warp_affine_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                                   const double M[6], float *dst, int dh, int dw, ptrdiff_t dst_stride_el)
{
    VKX_REQUIRE(ctx && src && M && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh >= 0 && dw >= 0, "bad shape");
    auto s = vkx_in(src, sh, sw, 1, src_stride_el), d = vkx_out(dst, dh, dw, 1, dst_stride_el);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_warp_affine_f32_dev(ctx, s.dev(), sh, sw, s.pitch, M, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_warp_perspective_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                                       const double M[9], uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && M && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh >= 0 && dw >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, cn, src_stride), d = vkx_out(dst, dh, dw, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_warp_perspective_u8_dev(ctx, s.dev(), sh, sw, cn, s.pitch, M, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_warp_perspective_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                                        const double M[9], float *dst, int dh, int dw, ptrdiff_t dst_stride_el)
{
    VKX_REQUIRE(ctx && src && M && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh >= 0 && dw >= 0, "bad shape");
    auto s = vkx_in(src, sh, sw, 1, src_stride_el), d = vkx_out(dst, dh, dw, 1, dst_stride_el);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_warp_perspective_f32_dev(ctx, s.dev(), sh, sw, s.pitch, M, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_grid_to_map(vkx_ctx *ctx, const int32_t *src_vertices, const int32_t *dst_vertices, int rows,
                               int cols, int dh, int dw, float *map_x, float *map_y, ptrdiff_t map_stride_el,
                               int32_t *owner)
{
    VKX_REQUIRE(ctx && src_vertices && dst_vertices && map_x && map_y, "NULL argument");
    VKX_REQUIRE(rows >= 2 && cols >= 2 && dh > 0 && dw > 0, "bad shape");
    const size_t n_vert = (size_t)rows * cols;
    auto sv = vkx_in(src_vertices, 1, n_vert, 2, 0), dv = vkx_in(dst_vertices, 1, n_vert, 2, 0);
    auto mx = vkx_out(map_x, dh, dw, 1, map_stride_el), my = vkx_out(map_y, dh, dw, 1, map_stride_el);
    auto ow = vkx_out(owner, dh, dw, 1, dw);          // optional
    return vkx_host_run(ctx, {&sv, &dv, &mx, &my, &ow}, [&] {
        return vkx_grid_to_map_dev(ctx, sv.dev(), dv.dev(), rows, cols, dh, dw, mx.dev(), my.dev(), mx.pitch, ow.dev());
    });
}

namespace {

// The elements of a multi-element remap ([sh, sw] -> [dh, dw]): their planes staged behind `first` (the call's own planes), and
// dev_call(elements) with the elements as the _dev form takes them (device pointers, dense strides).
template <class Call>
int run_elems(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw, int dh, int dw,
              std::initializer_list<vkx_host_plane_raw *> first, Call &&dev_call)
{
    std::vector<vkx_host_plane<uint8_t>> src(n_elems), dst(n_elems);      // as bytes: an element is uint8 or float32
    std::vector<vkx_host_plane_raw *> planes(first);
    for (int i = 0; i < n_elems; i++) {
        const vkx_elem &e = elems[i];
        const int esz = e.is_f32 ? 4 : 1;
        src[i] = vkx_in((const uint8_t *)e.src, sh, (size_t)sw * esz, e.cn, e.src_stride * esz);
        dst[i] = vkx_out((uint8_t *)e.dst, dh, (size_t)dw * esz, e.cn, e.dst_stride * esz);
        planes.push_back(&src[i]);
        planes.push_back(&dst[i]);
    }
    return vkx_host_run(ctx, planes.data(), planes.size(), [&] {
        std::vector<vkx_elem> de(elems, elems + n_elems);
        for (int i = 0; i < n_elems; i++) {
            de[i].src = src[i].dev();
            de[i].dst = dst[i].dev();
            de[i].src_stride = (ptrdiff_t)sw * de[i].cn;
            de[i].dst_stride = (ptrdiff_t)dw * de[i].cn;
        }
        return dev_call(de.data());
    });
}

} // namespace

VKX_EXPORT int vkx_grid_remap(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw,
                              const int32_t *src_vertices, const int32_t *dst_vertices, int rows, int cols, int dh, int dw)
{
    VKX_REQUIRE(ctx && elems && src_vertices && dst_vertices, "NULL argument");
    VKX_REQUIRE(n_elems >= 1 && n_elems <= 4, "1..4 elements per call");
    VKX_REQUIRE(rows >= 2 && cols >= 2 && dh > 0 && dw > 0 && sh > 0 && sw > 0, "bad shape");
    for (int i = 0; i < n_elems; i++) VKX_REQUIRE(elems[i].src && elems[i].dst && elems[i].cn >= 1 && elems[i].cn <= 4, "bad element");
    const size_t n_vert = (size_t)rows * cols;
    auto sv = vkx_in(src_vertices, 1, n_vert, 2, 0), dv = vkx_in(dst_vertices, 1, n_vert, 2, 0);
    return run_elems(ctx, elems, n_elems, sh, sw, dh, dw, {&sv, &dv}, [&](const vkx_elem *de) {
        return vkx_grid_remap_dev(ctx, de, n_elems, sh, sw, sv.dev(), dv.dev(), rows, cols, dh, dw);
    });
}

VKX_EXPORT int vkx_remap_multi(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw, const float *map_x,
                               const float *map_y, ptrdiff_t map_stride_el, int dh, int dw)
{
    VKX_REQUIRE(ctx && elems && map_x && map_y, "NULL argument");
    VKX_REQUIRE(n_elems >= 1 && n_elems <= 8, "1..8 elements per call");
    VKX_REQUIRE(dh >= 0 && dw >= 0 && sh > 0 && sw > 0, "bad shape");
    for (int i = 0; i < n_elems; i++) VKX_REQUIRE(elems[i].src && elems[i].dst && elems[i].cn >= 1 && elems[i].cn <= 4, "bad element");
    auto mx = vkx_in(map_x, dh, dw, 1, map_stride_el), my = vkx_in(map_y, dh, dw, 1, map_stride_el);
    return run_elems(ctx, elems, n_elems, sh, sw, dh, dw, {&mx, &my}, [&](const vkx_elem *de) {
        return vkx_remap_multi_dev(ctx, de, n_elems, sh, sw, mx.dev(), my.dev(), mx.pitch, dh, dw);
    });
}

VKX_EXPORT int vkx_gaussian_blur_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                    int ksize, double sigma, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_gaussian_blur_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, ksize, sigma, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_color_shift_rgb(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int delta,
                                   uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0, "bad shape");
    VKX_REQUIRE(src_stride == dst_stride, "host color_shift needs equal source / destination pitch");
    auto p = vkx_plane(src, dst, h, w, 3, src_stride);       // one device plane, shifted in place
    return vkx_host_run(ctx, {&p}, [&] {
        return vkx_color_shift_rgb_dev(ctx, p.dev(), h, w, p.pitch, delta, p.dev(), p.pitch);
    });
}

VKX_EXPORT int vkx_cvt_rgb_hsv_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int to_hsv,
                                  uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0, "bad shape");
    auto s = vkx_in(src, h, w, 3, src_stride), d = vkx_out(dst, h, w, 3, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_cvt_rgb_hsv_u8_dev(ctx, s.dev(), h, w, s.pitch, to_hsv, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_mean_shift_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int delta,
                                 int has_threshold, int threshold, int cycle, unsigned channel_mask, uint8_t *dst,
                                 ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_mean_shift_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, delta, has_threshold, threshold, cycle, channel_mask,
                                     d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_add_noise_i16(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                 const int16_t *noise, ptrdiff_t noise_stride_el, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && noise && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    auto n = vkx_in(noise, h, w, cn, noise_stride_el);
    return vkx_host_run(ctx, {&s, &n, &d}, [&] {
        return vkx_add_noise_i16_dev(ctx, s.dev(), h, w, cn, s.pitch, n.dev(), n.pitch, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_line_streak_u8(vkx_ctx *ctx, uint8_t *img, int h, int w, int cn, ptrdiff_t stride, int thickness,
                                  int gap, int dash_thickness, int dash_gap, const uint8_t color[4], double alpha,
                                  int enable_vert, int enable_hori)
{
    VKX_REQUIRE(ctx && img, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto p = vkx_inout(img, h, w, cn, stride);
    return vkx_host_run(ctx, {&p}, [&] {
        return vkx_line_streak_u8_dev(ctx, p.dev(), h, w, cn, p.pitch, thickness, gap, dash_thickness, dash_gap, color, alpha,
                                      enable_vert, enable_hori);
    });
}

#define VKX_TRY(expr)            \
    do {                         \
        int rc__ = (expr);       \
        if (rc__) return rc__;   \
    } while (0)

// Device page, host layer planes (the text lines of a page assembled onto a device-resident image): the planes are staged
// like vkx_fill_u8's, the page neither travels nor is waited for.  Asynchronous on the ctx stream.
VKX_EXPORT int vkx_fill_u8_dev_host_layers(vkx_ctx *ctx, uint8_t *dst_dev, int h, int w, int cn, ptrdiff_t dst_stride,
                                           const vkx_layer *layers, int n_layers)
{
    VKX_REQUIRE(ctx && dst_dev, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    VKX_REQUIRE(n_layers >= 0 && (n_layers == 0 || layers), "bad layer list");
    HostStage st(ctx);
    std::vector<int> mid(n_layers, -1), aid(n_layers, -1), vid(n_layers, -1);
    constexpr int kOnDevice = VKX_LAYER_MASK_ON_DEVICE | VKX_LAYER_ALPHA_ON_DEVICE | VKX_LAYER_VALUE_ON_DEVICE;
    // A layer selected by its alpha plane alone (fill_np_array: np_mask = alpha > 0, element/box.py:329-331) touches nothing in rows whose
    // alpha is <= 0 throughout: the box shrinks to the rows that select something (a page-sized score map with a bounding-box line or a
    // barcode in it -- page_assembler.py:167-177 -- is 4 MB of zeros around a few KB), so neither the CPU staging pass nor the link
    // carries them.  A dense plane costs the scan a few elements at its first and last row.
    std::vector<vkx_layer> cropped(layers, layers + n_layers);
    for (int i = 0; i < n_layers; i++) {
        vkx_layer &l = cropped[i];
        if (!l.alpha || l.mask || (l.mode & VKX_LAYER_ALPHA_ON_DEVICE) || l.height <= 0 || l.width <= 0) continue;
        auto selects = [&](int row) {
            const float *a = l.alpha + (ptrdiff_t)row * l.alpha_stride_el;
            // an all-zero row first, as one OR over its words (no early exit: the compiler vectorises it; a page-sized score map is
            // 4 MB of exactly that), then the exact test for rows that hold anything
            uint32_t any = 0;
            for (int x = 0; x < l.width; x++) {
                uint32_t bits;
                memcpy(&bits, a + x, 4);
                any |= bits;
            }
            if (!any) return false;
            for (int x = 0; x < l.width; x++)
                if (a[x] > 0.0f) return true;
            return false;
        };
        int r0 = 0, r1 = l.height;
        while (r0 < r1 && !selects(r0)) r0++;
        while (r1 > r0 && !selects(r1 - 1)) r1--;
        if (r0 == 0 && r1 == l.height) continue;
        if (r0 == r1) { l.height = 0; continue; }          // selects nothing: dropped by the composite (to_layer_dev)
        l.alpha += (ptrdiff_t)r0 * l.alpha_stride_el;
        if (l.value) l.value += (ptrdiff_t)r0 * l.value_stride;
        l.up += r0;
        l.height = r1 - r0;
    }
    layers = cropped.data();
    for (int i = 0; i < n_layers; i++) {
        const vkx_layer &l = layers[i];
        VKX_REQUIRE(l.height >= 0 && l.width >= 0, "bad layer box");
        if (l.mask && !(l.mode & VKX_LAYER_MASK_ON_DEVICE)) mid[i] = st.add(l.mask, nullptr, (size_t)l.width, l.height, l.mask_stride);
        if (l.alpha && !(l.mode & VKX_LAYER_ALPHA_ON_DEVICE)) aid[i] = st.add(l.alpha, nullptr, (size_t)l.width * 4, l.height, l.alpha_stride_el * 4);
        if (l.value && !(l.mode & VKX_LAYER_VALUE_ON_DEVICE)) vid[i] = st.add(l.value, nullptr, (size_t)l.width * cn, l.height, l.value_stride);
    }
    // Where the kernel finds the planes: a few KB (a mask strip, a small box) are read in place in the mapped ring -- no copy at all;
    // a page's worth (MBs) is copied to device memory by a DMA engine (commit(): one copy out of the ring) and read from HBM: the
    // composite kernel holding CUs for 0.6 ms while 16 MB cross the link was the largest kernel of a page (profiles/r6c_page_dispatches.txt)
    // and, with several workers on the GPU, compute-queue time is what the workers share.  VKX_LAYERS_MAPPED=1 / 0 forces one way.
    static const int map_env = vkx_env_on("VKX_LAYERS_MAPPED", -1);
    const bool mapped = map_env >= 0 ? map_env != 0 : st.total_bytes() <= ((size_t)64 << 10);
    if (!mapped || !st.commit_mapped()) VKX_TRY(st.commit(true));
    auto composite = [&] {
        std::vector<vkx_layer> dl(layers, layers + n_layers);
        for (int i = 0; i < n_layers; i++) {
            if (mid[i] >= 0) { dl[i].mask = st.dev<uint8_t>(mid[i]); dl[i].mask_stride = layers[i].width; }
            if (aid[i] >= 0) { dl[i].alpha = st.dev<float>(aid[i]); dl[i].alpha_stride_el = layers[i].width; }
            if (vid[i] >= 0) { dl[i].value = st.dev<uint8_t>(vid[i]); dl[i].value_stride = (ptrdiff_t)layers[i].width * cn; }
            dl[i].mode &= ~kOnDevice;
        }
        return vkx_fill_u8_dev(ctx, dst_dev, h, w, cn, dst_stride, dl.data(), n_layers);
    };
    int rc = composite();
    // the composite's tile tables did not fit behind the planes held in the ring (it takes them before its first launch):
    // the planes go to device memory instead, as above
    if (st.release_hold()) {
        VKX_TRY(st.commit(true));
        rc = composite();
    }
    return rc;
}

namespace {

// vkx_fill_u8 / vkx_fill_f32: the destination staged in place, every plane a layer has (mask, alpha, value) as an input, and
// dev_call(destination, layers) with the layers pointing to the dense device planes.  L: vkx_layer (uint8 values of cn channels)
// or vkx_layer_f32 (float32 values, one channel); value_stride: the value plane's stride field of L.
template <class T, class L, class Call>
int fill_host(vkx_ctx *ctx, T *dst, int h, int w, int cn, ptrdiff_t dst_stride, const L *layers, int n_layers,
              ptrdiff_t L::*value_stride, Call &&dev_call)
{
    auto d = vkx_inout(dst, h, w, cn, dst_stride);
    std::vector<vkx_host_plane<uint8_t>> m(n_layers);
    std::vector<vkx_host_plane<float>> a(n_layers);
    std::vector<vkx_host_plane<T>> v(n_layers);
    std::vector<vkx_host_plane_raw *> planes{&d};
    for (int i = 0; i < n_layers; i++) {
        const L &l = layers[i];
        m[i] = vkx_in(l.mask, l.height, l.width, 1, l.mask_stride);
        a[i] = vkx_in(l.alpha, l.height, l.width, 1, l.alpha_stride_el);
        v[i] = vkx_in(l.value, l.height, l.width, cn, l.*value_stride);
        planes.insert(planes.end(), {&m[i], &a[i], &v[i]});
    }
    return vkx_host_run(ctx, planes.data(), planes.size(), [&] {
        std::vector<L> dl(layers, layers + n_layers);
        for (int i = 0; i < n_layers; i++) {
            dl[i].mask = m[i].dev();
            dl[i].mask_stride = m[i].pitch;
            dl[i].alpha = a[i].dev();
            dl[i].alpha_stride_el = a[i].pitch;
            dl[i].value = v[i].dev();
            dl[i].*value_stride = v[i].pitch;
        }
        return dev_call(d, dl.data());
    });
}

} // namespace

VKX_EXPORT int vkx_fill_u8(vkx_ctx *ctx, uint8_t *dst, int h, int w, int cn, ptrdiff_t dst_stride,
                           const vkx_layer *layers, int n_layers)
{
    VKX_REQUIRE(ctx && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    VKX_REQUIRE(n_layers >= 0 && (n_layers == 0 || layers), "bad layer list");
    for (int i = 0; i < n_layers; i++) VKX_REQUIRE(layers[i].height >= 0 && layers[i].width >= 0, "bad layer box");
    return fill_host(ctx, dst, h, w, cn, dst_stride, layers, n_layers, &vkx_layer::value_stride,
                     [&](const vkx_host_plane<uint8_t> &d, const vkx_layer *dl) {
                         return vkx_fill_u8_dev(ctx, d.dev(), h, w, cn, d.pitch, dl, n_layers);
                     });
}

VKX_EXPORT int vkx_fill_f32(vkx_ctx *ctx, float *dst, int h, int w, ptrdiff_t dst_stride_el,
                            const vkx_layer_f32 *layers, int n_layers)
{
    VKX_REQUIRE(ctx && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0, "bad shape");
    VKX_REQUIRE(n_layers >= 0 && (n_layers == 0 || layers), "bad layer list");
    for (int i = 0; i < n_layers; i++) VKX_REQUIRE(layers[i].height >= 0 && layers[i].width >= 0, "bad layer box");
    return fill_host(ctx, dst, h, w, 1, dst_stride_el, layers, n_layers, &vkx_layer_f32::value_stride_el,
                     [&](const vkx_host_plane<float> &d, const vkx_layer_f32 *dl) {
                         return vkx_fill_f32_dev(ctx, d.dev(), h, w, d.pitch, dl, n_layers);
                     });
}

VKX_EXPORT int vkx_resize_cubic_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                                   uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, cn, src_stride), d = vkx_out(dst, dh, dw, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_resize_cubic_u8_dev(ctx, s.dev(), sh, sw, cn, s.pitch, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_resize_cubic_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el, float *dst,
                                    int dh, int dw, ptrdiff_t dst_stride_el)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, 1, src_stride_el), d = vkx_out(dst, dh, dw, 1, dst_stride_el);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_resize_cubic_f32_dev(ctx, s.dev(), sh, sw, s.pitch, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_resize_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el, float *dst, int dh, int dw,
                              ptrdiff_t dst_stride_el, int interpolation)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, 1, src_stride_el), d = vkx_out(dst, dh, dw, 1, dst_stride_el);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_resize_f32_dev(ctx, s.dev(), sh, sw, s.pitch, d.dev(), dh, dw, d.pitch, interpolation);
    });
}

VKX_EXPORT int vkx_filter2d_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                               const float *kernel_host, int kh, int kw, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_filter2d_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, kernel_host, kh, kw, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_pointwise_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int op, int p0,
                                int p1, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_pointwise_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, op, p0, p1, channel_mask, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_impulse_noise_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                    const uint8_t *selector, ptrdiff_t selector_stride, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && selector && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), m = vkx_in(selector, h, w, 1, selector_stride);
    auto d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &m, &d}, [&] {
        return vkx_impulse_noise_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, m.dev(), m.pitch, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_speckle_noise_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                    const double *noise, ptrdiff_t noise_stride_el, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && noise && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    auto n = vkx_in(noise, h, w, cn, noise_stride_el);
    return vkx_host_run(ctx, {&s, &n, &d}, [&] {
        return vkx_speckle_noise_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, n.dev(), n.pitch, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_cvt_color_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int code, uint8_t *dst,
                                ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0, "bad shape");
    const int scn = code == VKX_CVT_GRAY2RGB || code == VKX_CVT_GRAY2RGBA ? 1 : (code == VKX_CVT_RGBA2RGB || code == VKX_CVT_RGBA2GRAY ? 4 : 3);
    const int dcn = code == VKX_CVT_RGB2GRAY || code == VKX_CVT_RGBA2GRAY ? 1 : (code == VKX_CVT_RGB2RGBA || code == VKX_CVT_GRAY2RGBA ? 4 : 3);
    auto s = vkx_in(src, h, w, scn, src_stride), d = vkx_out(dst, h, w, dcn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_cvt_color_u8_dev(ctx, s.dev(), h, w, s.pitch, code, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_blend_u8(vkx_ctx *ctx, const uint8_t *a, ptrdiff_t a_stride, const uint8_t *b, ptrdiff_t b_stride, int h, int w,
                            int cn, double w0, double w1, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && a && b && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn >= 1 && cn <= 4, "bad shape");
    auto pa = vkx_in(a, h, w, cn, a_stride), pb = vkx_in(b, h, w, cn, b_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&pa, &pb, &d}, [&] {
        return vkx_blend_u8_dev(ctx, pa.dev(), pa.pitch, pb.dev(), pb.pitch, h, w, cn, w0, w1, channel_mask, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_fog_f32_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, const float *weight,
                              ptrdiff_t weight_stride_el, const float *fog, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && weight && fog && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn >= 1 && cn <= 4, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    auto m = vkx_in(weight, h, w, 1, weight_stride_el);
    return vkx_host_run(ctx, {&s, &m, &d}, [&] {
        return vkx_fog_f32_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, m.dev(), m.pitch, fog, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_brightness_shift_rgb(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int delta,
                                        uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0, "bad shape");
    auto s = vkx_in(src, h, w, 3, src_stride), d = vkx_out(dst, h, w, 3, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_brightness_shift_rgb_dev(ctx, s.dev(), h, w, s.pitch, delta, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_color_balance_rgb(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, double ratio,
                                     uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0, "bad shape");
    auto s = vkx_in(src, h, w, 3, src_stride), d = vkx_out(dst, h, w, 3, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_color_balance_rgb_dev(ctx, s.dev(), h, w, s.pitch, ratio, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_histogram_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int32_t *hist)
{
    VKX_REQUIRE(ctx && src && hist, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn >= 1 && cn <= 4, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride);
    auto d = vkx_out(hist, 1, 256, cn, 0);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_histogram_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, d.dev());
    });
}

VKX_EXPORT int vkx_apply_lut_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                const uint8_t *lut_host, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst && lut_host, "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && cn >= 1 && cn <= 4, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_apply_lut_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, lut_host, channel_mask, d.dev(), d.pitch);
    });
}

VKX_EXPORT int vkx_gather_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                             const int32_t *pos_y, const int32_t *pos_x, ptrdiff_t pos_stride_el, uint8_t *dst, int dh, int dw,
                             ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && pos_y && pos_x && dst, "NULL argument");
    VKX_REQUIRE(sh >= 0 && sw >= 0 && dh >= 0 && dw >= 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, cn, src_stride);
    auto py = vkx_in(pos_y, dh, dw, 1, pos_stride_el), px = vkx_in(pos_x, dh, dw, 1, pos_stride_el);
    auto d = vkx_out(dst, dh, dw, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &py, &px, &d}, [&] {
        return vkx_gather_u8_dev(ctx, s.dev(), sh, sw, cn, s.pitch, py.dev(), px.dev(), py.pitch, d.dev(), dh, dw, d.pitch);
    });
}

VKX_EXPORT int vkx_resize_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride, uint8_t *dst,
                             int dh, int dw, ptrdiff_t dst_stride, int interpolation)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, sh, sw, cn, src_stride), d = vkx_out(dst, dh, dw, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_resize_u8_dev(ctx, s.dev(), sh, sw, cn, s.pitch, d.dev(), dh, dw, d.pitch, interpolation);
    });
}

VKX_EXPORT int vkx_jpeg_roundtrip_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, uint8_t *dst,
                                     ptrdiff_t dst_stride, int quality)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h > 0 && w > 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_jpeg_roundtrip_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, d.dev(), d.pitch, quality);
    });
}

VKX_EXPORT int vkx_saturate_i64_u8(vkx_ctx *ctx, const int64_t *src, size_t n, uint8_t *dst)
{
    VKX_REQUIRE(ctx && (n == 0 || (src && dst)), "NULL argument");
    if (n == 0) return VKX_OK;
    auto s = vkx_in(src, 1, n, 1, 0);
    auto d = vkx_out(dst, 1, n, 1, 0);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_saturate_i64_u8_dev(ctx, s.dev(), n, d.dev());
    });
}

VKX_EXPORT int vkx_zoom_in_blur_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                   const int32_t *sizes_hw_host, int n_sizes, double alpha, uint8_t *dst, ptrdiff_t dst_stride)
{
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h > 0 && w > 0 && cn > 0, "bad shape");
    auto s = vkx_in(src, h, w, cn, src_stride), d = vkx_out(dst, h, w, cn, dst_stride);
    return vkx_host_run(ctx, {&s, &d}, [&] {
        return vkx_zoom_in_blur_u8_dev(ctx, s.dev(), h, w, cn, s.pitch, sizes_hw_host, n_sizes, alpha, d.dev(), d.pitch);
    });
}
