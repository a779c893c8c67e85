/*
 * vkx.h -- C ABI of libvkx.so: the MI355X (gfx950) implementation of vkit's per-pixel
 * distortion hot path.  This header is the drop-in boundary: it is what a binding on the
 * reference side (ctypes) loads instead of the cv2 / numpy calls cited
 * at each entry point.  Paths are relative to the reference's vkit/ package.
 *
 * Conventions
 *   - Every function returns 0 (VKX_OK) or a negative error code; vkx_last_error() returns a
 *     thread-local human readable message for the last failure on the calling thread.
 *   - A vkx_ctx owns one HIP stream and all device scratch of one (process, GPU) pair.  Calls
 *     on one ctx must be serialised by the caller.  ctypes releases the GIL around calls.
 *   - `*_dev` entry points take DEVICE pointers, enqueue on the ctx stream and return
 *     immediately (vkx_ctx_sync to wait).  Entry points without the suffix take HOST
 *     pointers, stage through ctx scratch and are synchronous; the library never retains a
 *     host pointer past the call.
 *   - Images are row-major, channel-interleaved; `*_stride` is the row pitch in BYTES for
 *     uint8 planes and in ELEMENTS for float32 / int16 / int32 planes (`*_stride_el`).  A stride is at least
 *     one row (width x channels); a shorter or negative one is VKX_ERR_INVALID before anything is launched, except
 *     on a single-row plane, whose stride is never used.  This holds for stride arguments and for the planes of
 *     vkx_elem, vkx_layer(_f32), vkx_paint_set, vkx_noise_plane and vkx_chain_item (src_stride, dst_stride, and noise_stride_el
 *     of a plane noise).  Entry points that cannot run in place (resize, remap, warps, blurs and
 *     filter2d, gather, the JPEG round trip, zoom_in_blur, channel-count conversions, the channel permutation, the chain: the
 *     src and dst of one vkx_chain_item) refuse a source and destination whose byte ranges overlap.  The chain checks every
 *     item of a batch before it queues anything.  What remains particular to vkx_chain_item: the fused kernel takes a source
 *     pitch below 2^24 bytes and planes whose byte offsets fit 32 bits (sh * src_stride + 8 and dh * dst_stride up to 2^32 - 1);
 *     items beyond that run through the per-stage kernels, with the same pixels.
 *   - Integer and byte results are bit-exact with oracle/ (the CPU restatement of the
 *     reference's numpy/OpenCV arithmetic); float32 results (ScoreMap) are bit-exact too,
 *     the stated tolerance against cv2 itself is 2 ulp.
 */
#ifndef VKX_H_
#define VKX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VKX_OK 0
#define VKX_ERR_INVALID (-1)     /* bad argument */
#define VKX_ERR_HIP (-2)         /* HIP runtime failure (message has the hipError string) */
#define VKX_ERR_NOMEM (-3)
#define VKX_ERR_UNSUPPORTED (-4)
#define VKX_ERR_OUT_OF_LATTICE (-5) /* a point falls outside the lattice cells (the reference raises IndexError there) */
#define VKX_ERR_DIVIDE (-6)         /* a division by zero the reference raises FloatingPointError for */
#define VKX_ERR_CHAR_MASK (-7)      /* a char the reference raises for (vkx_char_set.boxes_host has its status) */

typedef struct vkx_ctx vkx_ctx;

/* ---- context, stream, memory -------------------------------------------------------- */
int vkx_version(void);
const char *vkx_last_error(void);
int vkx_device_count(int *count);
/* "0000:c1:00.0" of visible device `device` (hipDeviceGetPCIBusId): process placement next to the GPU's NUMA node (vkit_amd/shard.py) */
int vkx_device_pci_bus_id(int device, char *buf, int len);
int vkx_ctx_create(int device, vkx_ctx **out);
int vkx_ctx_destroy(vkx_ctx *ctx);
int vkx_ctx_sync(vkx_ctx *ctx);
/* Borrow an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL restores
 * the ctx's own stream. */
int vkx_ctx_set_stream(vkx_ctx *ctx, void *hip_stream);
void *vkx_ctx_stream(vkx_ctx *ctx);
int vkx_malloc(vkx_ctx *ctx, size_t bytes, void **dptr);
int vkx_free(vkx_ctx *ctx, void *dptr);
int vkx_upload(vkx_ctx *ctx, void *dptr, const void *hptr, size_t bytes);   /* synchronous */
int vkx_download(vkx_ctx *ctx, void *hptr, const void *dptr, size_t bytes); /* synchronous */
int vkx_memset(vkx_ctx *ctx, void *dptr, int value, size_t bytes);          /* async */

/* ---- page-locked host memory, copy streams, ordering ----------------------------------------
 * For callers that keep host arrays flowing (the reference hands numpy arrays in and out of every operator,
 * mechanism/distortion/interface.py:824-912; its process pool, utility/pool.py:65-96, is the only overlap it has):
 * a ctx owns a host->device and a device->host copy stream next to its compute stream.  vkx_upload_async /
 * vkx_download_async enqueue on those; vkx_ctx_order(later, earlier) makes `later` wait for everything queued on
 * `earlier` at the time of the call; vkx_event_record / vkx_event_wait let the host wait for one point of one stream.
 * Copies overlap compute only from / to page-locked memory (vkx_host_alloc). */
#define VKX_STREAM_COMPUTE 0
#define VKX_STREAM_COPY_IN 1
#define VKX_STREAM_COPY_OUT 2
int vkx_host_alloc(vkx_ctx *ctx, size_t bytes, void **hptr);
int vkx_host_free(vkx_ctx *ctx, void *hptr);
int vkx_upload_async(vkx_ctx *ctx, void *dptr, const void *hptr, size_t bytes);
int vkx_download_async(vkx_ctx *ctx, void *hptr, const void *dptr, size_t bytes);
/* one copy on the named stream of the ctx: to_device 0 = device -> host, 1 = host -> device, 2 = device -> device */
int vkx_memcpy_async(vkx_ctx *ctx, int stream, void *dst, const void *src, size_t bytes, int to_device);
int vkx_ctx_order(vkx_ctx *ctx, int later_stream, int earlier_stream);
/* Ordering against a stream the context does not own (the consumer's: torch.cuda.current_stream().cuda_stream), for memory the
 * two share without a copy (vkit_amd/torch_bridge.py).  vkx_ctx_wait_external: the context's compute stream continues after
 * everything queued on `hip_stream` at the time of the call; vkx_ctx_signal_external: `hip_stream` continues after everything
 * queued on the context's compute stream at the time of the call.  Each is one event record and one hipStreamWaitEvent (the
 * event comes from the context's pool and returns to it on every exit); the host never waits.  hip_stream == NULL names the
 * LEGACY DEFAULT STREAM (handle 0, torch's default stream) -- unlike vkx_ctx_set_stream, where NULL means "restore".  Nothing
 * is queued when `hip_stream` is the compute stream itself.  Refused before anything is queued: a NULL ctx and a stream of
 * another device than the context's (VKX_ERR_INVALID); either stream in capture (VKX_ERR_UNSUPPORTED: a captured graph
 * cannot carry an ordering against work outside it). */
int vkx_ctx_wait_external(vkx_ctx *ctx, void *hip_stream);
int vkx_ctx_signal_external(vkx_ctx *ctx, void *hip_stream);
int vkx_ctx_sync_stream(vkx_ctx *ctx, int stream);
int vkx_event_record(vkx_ctx *ctx, int stream, void **event);
int vkx_event_wait(vkx_ctx *ctx, void *event);   /* waits on the host and releases the event */

/* ---- backward-map bilinear remap ----------------------------------------------------
 * cv.remap(src, map_x, map_y, cv.INTER_LINEAR), BORDER_CONSTANT 0
 *   mechanism/distortion/geometric/grid_rendering/grid_blender.py:60 (Image), :80 (Mask,
 *   bilinear on 0/1 bytes), :70 (ScoreMap).  cn in {1,3,4} for uint8. */
int vkx_remap_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                     const float *map_x, const float *map_y, ptrdiff_t map_stride_el,
                     uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_remap_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                      const float *map_x, const float *map_y, ptrdiff_t map_stride_el,
                      float *dst, int dh, int dw, ptrdiff_t dst_stride_el);
int vkx_remap_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                 const float *map_x, const float *map_y, ptrdiff_t map_stride_el,
                 uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_remap_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                  const float *map_x, const float *map_y, ptrdiff_t map_stride_el,
                  float *dst, int dh, int dw, ptrdiff_t dst_stride_el);

/* ---- affine / perspective warps -----------------------------------------------------
 * cv.warpAffine(mat, trans_mat, dsize) / cv.warpPerspective(mat, trans_mat, dsize)
 *   mechanism/distortion/geometric/affine.py:38-43 (affine_mat), used by :430-456.
 * M is the FORWARD matrix (row-major 2x3 / 3x3, float32-valued doubles), dsize = (dw, dh). */
int vkx_warp_affine_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                           const double M[6], uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_warp_affine_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                            const double M[6], float *dst, int dh, int dw, ptrdiff_t dst_stride_el);
int vkx_warp_perspective_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                                const double M[9], uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_warp_perspective_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                                 const double M[9], float *dst, int dh, int dw, ptrdiff_t dst_stride_el);
int vkx_warp_affine_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                       const double M[6], uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_warp_affine_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                        const double M[6], float *dst, int dh, int dw, ptrdiff_t dst_stride_el);
int vkx_warp_perspective_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                            const double M[9], uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_warp_perspective_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                             const double M[9], float *dst, int dh, int dw, ptrdiff_t dst_stride_el);

/* ---- image-grid distortions: grid -> dense map, and the fused grid remap ------------
 * ImageGrid.generate_remap_params  grid_rendering/type.py:209-261 with get_inv_trans_mat
 * (:182-197, cv.getPerspectiveTransform DECOMP_SVD) and the per-cell cv.fillPoly raster
 * (:199-207, element/polygon.py:70-77).  Vertices: int32 [rows, cols, 2] as (x, y), the ROUNDED
 * grid points of the source / destination ImageGrid.  Unfilled pixels map to (0, 0).
 * owner (optional): int32 [dh, dw], 1 + row-major index of the cell that wrote the pixel. */
int vkx_grid_to_map_dev(vkx_ctx *ctx, const int32_t *src_vertices, const int32_t *dst_vertices, int rows,
                        int cols, int dh, int dw, float *map_x, float *map_y, ptrdiff_t map_stride_el,
                        int32_t *owner);
int vkx_grid_to_map(vkx_ctx *ctx, const int32_t *src_vertices, const int32_t *dst_vertices, int rows,
                    int cols, int dh, int dw, float *map_x, float *map_y, ptrdiff_t map_stride_el,
                    int32_t *owner);

/* Shared-grid multi-element remap (blend_src_to_dst_{image,mask,score_map},
 * grid_blender.py:54-81 through one DistortionStateImageGridBased): the dense map is never
 * written to memory; every element is gathered in the same pass. */
typedef struct vkx_elem {
    const void *src;      /* uint8 [sh, sw, cn] or float32 [sh, sw] */
    void *dst;            /* same type, [dh, dw(, cn)] */
    ptrdiff_t src_stride; /* bytes (uint8) / elements (float32) */
    ptrdiff_t dst_stride;
    int32_t cn;           /* 1, 3, 4 for uint8; 1 for float32 */
    int32_t is_f32;       /* 0: uint8, 1: float32 */
} vkx_elem;
int vkx_grid_remap_dev(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw,
                       const int32_t *src_vertices, const int32_t *dst_vertices, int rows, int cols,
                       int dh, int dw);
/* The same elements through an explicit dense map shared by all of them (cv.remap per element with one
 * (map_x, map_y) pair, grid_blender.py:54-81 when the caller keeps the map of generate_remap_params). */
int vkx_remap_multi_dev(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw, const float *map_x,
                        const float *map_y, ptrdiff_t map_stride_el, int dh, int dw);
int vkx_remap_multi(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw, const float *map_x,
                    const float *map_y, ptrdiff_t map_stride_el, int dh, int dw);
int vkx_grid_remap(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw,
                   const int32_t *src_vertices, const int32_t *dst_vertices, int rows, int cols,
                   int dh, int dw);

/* ---- photometric members ------------------------------------------------------------ */
/* cv.GaussianBlur(mat, (k, k), sigma), BORDER_REFLECT_101  photometric/blur.py:54-69 */
int vkx_gaussian_blur_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                             int ksize, double sigma, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_gaussian_blur_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                         int ksize, double sigma, uint8_t *dst, ptrdiff_t dst_stride);
/* color_shift on RGB: cvtColor RGB2HSV_FULL, H = (H + delta) mod 256, HSV2RGB_FULL
 *   photometric/color.py:93-116, element/image.py:188-202,771-814.  In place allowed. */
int vkx_color_shift_rgb_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int delta,
                            uint8_t *dst, ptrdiff_t dst_stride);
int vkx_color_shift_rgb(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int delta,
                        uint8_t *dst, ptrdiff_t dst_stride);
/* cv.cvtColor(.., COLOR_RGB2HSV_FULL / COLOR_HSV2RGB_FULL)  element/image.py:794-808 */
int vkx_cvt_rgb_hsv_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int to_hsv,
                           uint8_t *dst, ptrdiff_t dst_stride);
int vkx_cvt_rgb_hsv_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int to_hsv,
                       uint8_t *dst, ptrdiff_t dst_stride);
/* _mean_shift  photometric/color.py:32-55 + photometric/opt.py:41-57.  channel_mask 0 = all. */
int vkx_mean_shift_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                          int delta, int has_threshold, int threshold, int cycle, unsigned channel_mask,
                          uint8_t *dst, ptrdiff_t dst_stride);
int vkx_mean_shift_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                      int delta, int has_threshold, int threshold, int cycle, unsigned channel_mask,
                      uint8_t *dst, ptrdiff_t dst_stride);
/* gaussion_noise_image tail: clip(int16(px) + noise, 0, 255)  photometric/noise.py:51-53.
 * noise: int16 [h, w, cn] = round(rng.normal(0, std, shape)), C order. */
int vkx_add_noise_i16_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                          const int16_t *noise, ptrdiff_t noise_stride_el, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_add_noise_i16(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                      const int16_t *noise, ptrdiff_t noise_stride_el, uint8_t *dst, ptrdiff_t dst_stride);
/* line_streak_image  photometric/streak.py:56-99 (+ :24-41), in place. */
int vkx_line_streak_u8_dev(vkx_ctx *ctx, uint8_t *img, int h, int w, int cn, ptrdiff_t stride, int thickness,
                           int gap, int dash_thickness, int dash_gap, const uint8_t color[4], double alpha,
                           int enable_vert, int enable_hori);
int vkx_line_streak_u8(vkx_ctx *ctx, uint8_t *img, int h, int w, int cn, ptrdiff_t stride, int thickness,
                       int gap, int dash_thickness, int dash_gap, const uint8_t color[4], double alpha,
                       int enable_vert, int enable_hori);

/* ellipse_streak  photometric/streak.py:283-337.  vkx_ellipse_mask_u8: the loop of
 * cv.ellipse(mask, (cx, cy), axes[i], angle 0, arc 0..360, color 1, thickness) calls (:312-324; LINE_8, shift 0) drawn
 * onto `mask` (uint8 [h, w]; touched pixels become 1, the others keep their value).  axes_host: HOST int32
 * [n_ellipses, 2] as (box.width // 2, box.height // 2).  thickness in 1 .. 32767 (filled ellipses are not on the path).
 * vkx_ellipse_streak_u8: that mask on a cleared plane, then Mask.fill_image(image, color, alpha) in place. */
int vkx_ellipse_mask_u8_dev(vkx_ctx *ctx, uint8_t *mask, ptrdiff_t mask_stride, int h, int w, int cx, int cy,
                            const int32_t *axes_host, int n_ellipses, int thickness);
int vkx_ellipse_mask_u8(vkx_ctx *ctx, uint8_t *mask, ptrdiff_t mask_stride, int h, int w, int cx, int cy,
                        const int32_t *axes_host, int n_ellipses, int thickness);
int vkx_ellipse_streak_u8_dev(vkx_ctx *ctx, uint8_t *img, int h, int w, int cn, ptrdiff_t stride, int cx, int cy,
                              const int32_t *axes_host, int n_ellipses, int thickness, const uint8_t color[4],
                              double alpha);
int vkx_ellipse_streak_u8(vkx_ctx *ctx, uint8_t *img, int h, int w, int cn, ptrdiff_t stride, int cx, int cy,
                          const int32_t *axes_host, int n_ellipses, int thickness, const uint8_t color[4],
                          double alpha);

/* cv.cvtColor on uint8 images, the codes Image.to_target_mode_image uses (element/image.py:188-202,771-814).
 * HSL images of the reference are HLS with the last two channels swapped on the host. */
#define VKX_CVT_RGB2HSV_FULL 0
#define VKX_CVT_HSV2RGB_FULL 1
#define VKX_CVT_RGB2HLS_FULL 2
#define VKX_CVT_HLS2RGB_FULL 3
#define VKX_CVT_RGB2GRAY 4   /* [h, w, 3] -> [h, w]; not in place */
#define VKX_CVT_GRAY2RGB 5   /* [h, w] -> [h, w, 3]; not in place */
#define VKX_CVT_RGBA2RGB 6   /* [h, w, 4] -> [h, w, 3]: alpha dropped; not in place */
#define VKX_CVT_RGB2RGBA 7   /* [h, w, 3] -> [h, w, 4]: alpha 255 */
#define VKX_CVT_GRAY2RGBA 8  /* [h, w] -> [h, w, 4] */
#define VKX_CVT_RGBA2GRAY 9  /* [h, w, 4] -> [h, w] */
int vkx_cvt_color_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int code,
                         uint8_t *dst, ptrdiff_t dst_stride);
int vkx_cvt_color_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int code,
                     uint8_t *dst, ptrdiff_t dst_stride);
/* color_balance on any image mode  photometric/color.py:371-396: dst = uint8(clip(w0 * a + w1 * b, 0, 255)) on the channels of
 * channel_mask (0 = all), b elsewhere; a = the grey version of the image in the image's own mode, b = the image, w0 = 1 - ratio,
 * w1 = ratio (float32 products rounded separately, truncation). */
int vkx_blend_u8_dev(vkx_ctx *ctx, const uint8_t *a, ptrdiff_t a_stride, const uint8_t *b, ptrdiff_t b_stride, int h, int w,
                     int cn, double w0, double w1, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_blend_u8(vkx_ctx *ctx, const uint8_t *a, ptrdiff_t a_stride, const uint8_t *b, ptrdiff_t b_stride, int h, int w, int cn,
                 double w0, double w1, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride);
/* fog with fractional fog values (GRAYSCALE images)  photometric/effect.py:192-205: dst = uint8(clip((1 - m) * px + m * fog[c]))
 * with the float32 weight plane m [h, w]; `fog`: cn float32 values on the host. */
int vkx_fog_f32_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, const float *weight,
                       ptrdiff_t weight_stride_el, const float *fog, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_fog_f32_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, const float *weight,
                   ptrdiff_t weight_stride_el, const float *fog, uint8_t *dst, ptrdiff_t dst_stride);
/* brightness_shift on RGB with the default HSL intermediate  photometric/color.py:125-160: RGB2HLS_FULL,
 * L = clip(L + delta), HLS2RGB_FULL, one pass.  In place allowed. */
int vkx_brightness_shift_rgb_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int delta,
                                 uint8_t *dst, ptrdiff_t dst_stride);
int vkx_brightness_shift_rgb(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, int delta,
                             uint8_t *dst, ptrdiff_t dst_stride);
/* color_balance on RGB  photometric/color.py:364-397: uint8(clip(fl32(1 - ratio) * gray + fl32(ratio) * px)),
 * gray = RGB2GRAY of the pixel.  In place allowed. */
int vkx_color_balance_rgb_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, double ratio,
                              uint8_t *dst, ptrdiff_t dst_stride);
int vkx_color_balance_rgb(vkx_ctx *ctx, const uint8_t *src, int h, int w, ptrdiff_t src_stride, double ratio,
                          uint8_t *dst, ptrdiff_t dst_stride);

/* complement / posterization / channel_permutation  photometric/color.py:299-357, 423-432 (numpy only).
 *   VKX_POINT_COMPLEMENT  p0 = threshold or -1 (none), p1 = enable_threshold_lte: v = 255 - v where selected
 *   VKX_POINT_POSTERIZE   p0 = num_bits in [0, 7]: v &= (0xFF >> p0) << p0
 *   VKX_POINT_PERMUTE     p0 = permutation, 2 bits per output channel: out[c] = in[(p0 >> 2c) & 3]; not in place
 * channel_mask 0 = all channels (ignored by PERMUTE). */
#define VKX_POINT_COMPLEMENT 0
#define VKX_POINT_POSTERIZE 1
#define VKX_POINT_PERMUTE 2
int vkx_pointwise_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int op, int p0,
                         int p1, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_pointwise_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int op, int p0,
                     int p1, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride);

/* The two halves of boundary_equalization / histogram_equalization  photometric/color.py:214-285:
 *   vkx_histogram_u8  per-channel histogram int32 [cn][256] (exact integer reduction; device pointer for *_dev)
 *   vkx_apply_lut_u8  dst[c] = lut[c][src[c]] on the channels of channel_mask (0 = all); lut is a HOST uint8 [cn][256]
 * Between them the host turns the histogram into the table: min / max and the float32 scale for the boundary
 * equalisation (numpy arithmetic of :222-243 per distinct value), cv.equalizeHist's cumulative table for the other. */
int vkx_histogram_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int32_t *hist);
int vkx_histogram_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, int32_t *hist);
/* std_shift's mean (photometric/color.py:165-210): sums_host [n_sel] = the float32 sums numpy forms inside np.mean of the float32
 * copy, value for value, including the roundings once a running sum has left the exactly representable range (2^24):
 *   sequential = 0  np.mean(mat) of a single plane, and the channels picked with mat[:, :, channels] (numpy lays that copy out
 *                   channel first): per channel, pieces of 8 192 contiguous elements summed exactly, accumulated in float32 one
 *                   after the other;
 *   sequential = 1  np.mean(mat.reshape(-1, C), axis=0) of ALL C >= 2 channels of an interleaved image: a sequential float32
 *                   accumulation over the pixels, per channel.
 * The mean is sums / float32(h * w).  h * w <= 2^22.  Synchronous (the caller builds its tables from the values); *_dev: src is a
 * device plane. */
int vkx_sum_f32_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, const int32_t *channels_host,
                       int n_sel, int sequential, float *sums_host);
int vkx_sum_f32_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride, const int32_t *channels_host,
                   int n_sel, int sequential, float *sums_host);
int vkx_apply_lut_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                         const uint8_t *lut_host, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride);
/* The same look-up for up to 8 dense single-channel device planes, each with its own HOST table uint8 [256], in one launch (the four masks
 * PageResizingStep binarises before and after their resize: Mask.to_resized_mask, element/mask.py:454-479). */
typedef struct vkx_lut_plane {
    const uint8_t *src;   /* device, dense, 16-byte aligned */
    uint8_t *dst;         /* device, dense, 16-byte aligned (may equal src) */
    size_t n_bytes;
    const uint8_t *lut_host;
} vkx_lut_plane;
int vkx_apply_lut_u8_planes_dev(vkx_ctx *ctx, const vkx_lut_plane *planes, int n_planes);
int vkx_apply_lut_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                     const uint8_t *lut_host, unsigned channel_mask, uint8_t *dst, ptrdiff_t dst_stride);

/* mat[pos_y, pos_x] -- numpy advanced indexing with two int32 index planes [dh, dw]: the pixel shuffle of
 * glass_blur  photometric/blur.py:204-250 (the planes come from the caller's numpy Generator stream).  Entries outside
 * the source are an error (VKX_ERR_INVALID). */
int vkx_gather_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                      const int32_t *pos_y, const int32_t *pos_x, ptrdiff_t pos_stride_el, uint8_t *dst, int dh, int dw,
                      ptrdiff_t dst_stride);
int vkx_gather_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                  const int32_t *pos_y, const int32_t *pos_x, ptrdiff_t pos_stride_el, uint8_t *dst, int dh, int dw,
                  ptrdiff_t dst_stride);

/* poisson_noise  photometric/noise.py:81-91: np.clip(samples, 0, 255).astype(uint8) of the int64 rng.poisson draws
 * (the draws themselves are the caller's numpy Generator stream; n values, flat). */
int vkx_saturate_i64_u8_dev(vkx_ctx *ctx, const int64_t *src, size_t n, uint8_t *dst);
int vkx_saturate_i64_u8(vkx_ctx *ctx, const int64_t *src, size_t n, uint8_t *dst);

/* impulse_noise  photometric/noise.py:125-150: selector uint8 [h, w] (0 keep, 1 salt = 255, 2 pepper = 0 on every
 * channel of the pixel), drawn by the caller's numpy Generator (rng.choice). */
int vkx_impulse_noise_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                             const uint8_t *selector, ptrdiff_t selector_stride, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_impulse_noise_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                         const uint8_t *selector, ptrdiff_t selector_stride, uint8_t *dst, ptrdiff_t dst_stride);

/* speckle_noise  photometric/noise.py:172-183: uint8(clip(px + px * noise, 0, 255)) evaluated in float64, noise
 * float64 [h, w, cn] = rng.normal(0, std, shape) of the caller's numpy Generator. */
int vkx_speckle_noise_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                             const double *noise, ptrdiff_t noise_stride_el, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_speckle_noise_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                         const double *noise, ptrdiff_t noise_stride_el, uint8_t *dst, ptrdiff_t dst_stride);

/* ---- alpha composite ----------------------------------------------------------------
 * fill_np_array  element/opt.py:118-209 reached through Box.fill_np_array element/box.py:311-340
 * (Box.fill_image :394-416, Mask.fill_image element/mask.py:601-612, ScoreMap.fill_image
 * element/score_map.py:678-687); layer order = PageAssemblerStep.run
 * pipeline/text_detection/page_assembler.py:155-236.  Layers are applied in order, in place.
 * All plane pointers of a layer live in the same memory space as dst (device for *_dev). */
typedef struct vkx_layer {
    int32_t up, left, height, width; /* box inside dst */
    const uint8_t *mask;             /* optional [height, width] uint8: selected where > 0 */
    ptrdiff_t mask_stride;
    const float *alpha;              /* optional [height, width] float32; selects alpha > 0 if !mask */
    ptrdiff_t alpha_stride_el;
    double alpha_scalar;             /* used when alpha == NULL; must be in [0, 1] */
    const uint8_t *value;            /* optional [height, width, cn] uint8 */
    ptrdiff_t value_stride;
    uint8_t value_const[4];          /* used when value == NULL */
    int32_t mode;                    /* VKX_FILL_*: keep_max_value / keep_min_value, element/opt.py:150-158 */
} vkx_layer;
#define VKX_FILL_PLAIN 0
#define VKX_FILL_KEEP_MAX 1 /* write only where dst < value; acts when alpha is the scalar 1.0, like the reference */
#define VKX_FILL_KEEP_MIN 2 /* write only where dst > value */
int vkx_fill_u8_dev(vkx_ctx *ctx, uint8_t *dst, int h, int w, int cn, ptrdiff_t dst_stride,
                    const vkx_layer *layers, int n_layers);
int vkx_fill_u8(vkx_ctx *ctx, uint8_t *dst, int h, int w, int cn, ptrdiff_t dst_stride,
                const vkx_layer *layers, int n_layers);
/* device page, HOST layer planes (page_assembler.py:155-236 onto a device-resident page): the planes are staged for the
 * call -- gathered in the context's page-locked ring and read THERE by the composite kernel (every plane byte is read once: no
 * copy to device memory, no copy dispatch) --, the page stays where it is; asynchronous.  A plane whose VKX_LAYER_*_ON_DEVICE bit
 * is or-ed into `mode` already lives in device memory and is used where it is (fill_page_inactive_region: a device mask selects,
 * the host bottom layer is the value). */
#define VKX_LAYER_MASK_ON_DEVICE 0x100
#define VKX_LAYER_ALPHA_ON_DEVICE 0x200
#define VKX_LAYER_VALUE_ON_DEVICE 0x400
int vkx_fill_u8_dev_host_layers(vkx_ctx *ctx, uint8_t *dst_dev, int h, int w, int cn, ptrdiff_t dst_stride,
                                const vkx_layer *layers_host_planes, int n_layers);
/* The layer lists of n_pages equally shaped device destinations in ONE launch (a batch of pages assembled together,
 * PageAssemblerStep.run per page of the batch): page p takes layers[layer_begin[p] .. layer_begin[p + 1]) in order, with the
 * pixels vkx_fill_u8_dev(dsts[p], ...) would produce.  dsts_host: HOST array of n_pages device pointers; layer_begin_host:
 * HOST int32 [n_pages + 1], layer_begin[0] == 0. */
int vkx_fill_u8_batch_dev(vkx_ctx *ctx, uint8_t *const *dsts_host, int n_pages, int h, int w, int cn, ptrdiff_t dst_stride,
                          const vkx_layer *layers, const int32_t *layer_begin_host);

/* float32 destinations: ScoreMap fills (Box.fill_score_map element/box.py:368-392, Mask.fill_score_map
 * element/mask.py:575-599, Polygon.fill_score_map element/polygon.py:475-487), the label height maps of
 * pipeline/text_detection/page_distortion.py:163-314. */
typedef struct vkx_layer_f32 {
    int32_t up, left, height, width;
    const uint8_t *mask;
    ptrdiff_t mask_stride;
    const float *alpha;
    ptrdiff_t alpha_stride_el;
    double alpha_scalar;
    const float *value;              /* optional [height, width] float32 */
    ptrdiff_t value_stride_el;
    float value_const;
    int32_t mode;
} vkx_layer_f32;
int vkx_fill_f32_dev(vkx_ctx *ctx, float *dst, int h, int w, ptrdiff_t dst_stride_el,
                     const vkx_layer_f32 *layers, int n_layers);
int vkx_fill_f32(vkx_ctx *ctx, float *dst, int h, int w, ptrdiff_t dst_stride_el,
                 const vkx_layer_f32 *layers, int n_layers);

/* ---- bicubic resize ------------------------------------------------------------------
 * cv.resize(mat, (dw, dh), interpolation=cv.INTER_CUBIC): Image.to_resized_image element/image.py:836-852
 * (bottom layer of fill_page_inactive_region, pipeline/text_detection/page_distortion.py:146-161),
 * Mask.to_resized_mask element/mask.py:454-479 (on the 0/255 plane), ScoreMap.to_resized_score_map
 * element/score_map.py:616-640.  Keys cubic A = -0.75, replicated border, 11-bit fixed-point coefficients and
 * (sum + 2^21) >> 22 rounding for uint8 (OpenCV's scalar path); float32 sums left to right. */
int vkx_resize_cubic_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                            uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_resize_cubic_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                             float *dst, int dh, int dw, ptrdiff_t dst_stride_el);
int vkx_resize_cubic_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                        uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride);
int vkx_resize_cubic_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el,
                         float *dst, int dh, int dw, ptrdiff_t dst_stride_el);

/* cv.resize with the interpolation codes of cv2 (NEAREST 0, LINEAR 1, CUBIC 2) on uint8: pixelation
 * photometric/effect.py:61-79 shrinks with INTER_LINEAR and grows back with INTER_NEAREST.  LINEAR: 11-bit
 * coefficients, OpenCV's two-stage vertical rounding, an exact 2 x 2 shrink is the INTER_AREA box. */
#define VKX_INTER_NEAREST 0
#define VKX_INTER_LINEAR 1
#define VKX_INTER_CUBIC 2
/* ... and the interpolations PageResizingStep samples for the page Image, Masks and ScoreMaps
 * (pipeline/text_detection/page_resizing.py:110-181, sample_cv_resize_interpolation utility/opt.py:125-148):
 * LANCZOS4 (8 x 8 taps, 11-bit coefficients / float32), LINEAR_EXACT (8.8 fixed point on uint8; float32 has no
 * bit-exact path in cv.resize and falls back to LINEAR), NEAREST_EXACT (16.16 index steps), AREA (shrinking only: box
 * sums for integer factors, fractional cell weights in float32 otherwise). */
#define VKX_INTER_AREA 3
#define VKX_INTER_LANCZOS4 4
#define VKX_INTER_LINEAR_EXACT 5
#define VKX_INTER_NEAREST_EXACT 6
int vkx_resize_u8_dev(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                      uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride, int interpolation);
int vkx_resize_u8(vkx_ctx *ctx, const uint8_t *src, int sh, int sw, int cn, ptrdiff_t src_stride,
                  uint8_t *dst, int dh, int dw, ptrdiff_t dst_stride, int interpolation);

/* jpeg_quality photometric/effect.py:41-42: cv.imdecode(cv.imencode('.jpeg', mat, [IMWRITE_JPEG_QUALITY, quality])) as
 * libjpeg-turbo computes it (baseline tables scaled by jpeg_set_quality, 4:2:0, accurate integer DCT, fancy upsampling).
 * cn 3: the mat is BGR to the codec (channel 2 carries the R weight); cn 1: a one-component (grayscale) JPEG.  quality
 * 0 .. 100 (0 scales as 1).  Two launches; the decoded planes live in context scratch between them (cn 3 only). */
int vkx_jpeg_roundtrip_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                              uint8_t *dst, ptrdiff_t dst_stride, int quality);
int vkx_jpeg_roundtrip_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                          uint8_t *dst, ptrdiff_t dst_stride, int quality);

/* cv.filter2D(image, -1, kernel) on uint8 with a float32 kernel of up to 15 x 15 taps (HOST pointer, row-major):
 * defocus_blur / motion_blur  photometric/blur.py:85-192.  Correlation anchored at the kernel centre,
 * BORDER_REFLECT_101, the non-zero taps in row-major order accumulated in float32 (products and sums rounded
 * separately), cvRound + saturate. */
int vkx_filter2d_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                        const float *kernel_host, int kh, int kw, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_filter2d_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                    const float *kernel_host, int kh, int kw, uint8_t *dst, ptrdiff_t dst_stride);

/* the same on a float32 plane (ScoreMap.to_resized_score_map element/score_map.py:616-640); strides in elements */
int vkx_resize_f32_dev(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el, float *dst, int dh, int dw,
                       ptrdiff_t dst_stride_el, int interpolation);
int vkx_resize_f32(vkx_ctx *ctx, const float *src, int sh, int sw, ptrdiff_t src_stride_el, float *dst, int dh, int dw,
                   ptrdiff_t dst_stride_el, int interpolation);

/* zoom_in_blur  photometric/blur.py:264-316: the image plus the centred crops of its INTER_CUBIC enlargements to the
 * sizes of sizes_hw_host (HOST int32 [n, 2] as (height, width), every size >= the image) are summed in uint16, then
 * dst = uint8(clip((1 - alpha) * px + alpha * rint(sum / (n + 1)))) in float64. */
int vkx_zoom_in_blur_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                            const int32_t *sizes_hw_host, int n_sizes, double alpha, uint8_t *dst, ptrdiff_t dst_stride);
int vkx_zoom_in_blur_u8(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                        const int32_t *sizes_hw_host, int n_sizes, double alpha, uint8_t *dst, ptrdiff_t dst_stride);

/* ---- point projection through the lattice ------------------------------------------------
 * FuncImageGridBased.func_point, grid_rendering/interface.py:194-216, for a batch of points (the reference loops
 * point by point, distortion/interface.py:638-661): cell = (y // grid_size, x // grid_size) of the ROUNDED point,
 * trans_mat = cv.getPerspectiveTransform(src quad, dst quad) of that cell (grid_rendering/type.py:166-180),
 * (x', y') = trans_mat . (smooth_x, smooth_y, 1) dehomogenised, all in float64.  Everything is HOST memory:
 * src_vertices / dst_vertices int32 [rows, cols, 2] (x, y); pts_xy int32 [n, 2] rounded (x, y); pts_smooth_xy
 * float64 [n, 2]; out_xy float64 [n, 2].  A point whose cell index falls outside the (rows-1) x (cols-1) cells is an
 * error (VKX_ERR_OUT_OF_LATTICE; the reference raises IndexError there). */
int vkx_grid_project_points(vkx_ctx *ctx, const int32_t *src_vertices, const int32_t *dst_vertices, int rows, int cols,
                            int grid_size, const int32_t *pts_xy, const double *pts_smooth_xy, int n, double *out_xy);

/* ---- similarity_mls lattice construction --------------------------------------------------
 * SimilarityMlsPointProjector.project_point, geometric/mls.py:38-135, for every vertex of the source lattice in one
 * launch (the reference projects vertex by vertex through create_dst_image_grid_and_shift_amounts_and_resize_ratios,
 * grid_rendering/grid_creator.py:44-115).  float32 arithmetic in the reference's order of operations, including the
 * accumulation orders of numpy's reductions and of np.matmul (csrc/mls.hip lists them).
 *   src_handles / dst_handles                float32 [n_handles, 2] (x, y): the INTEGER handle positions
 *                                            (PointTuple.to_smooth_np_array, element/point.py:251-252)
 *   src_handles_smooth / dst_handles_smooth  float64 [n_handles, 2]: a vertex exactly on a source handle maps to that
 *                                            handle's target (mls.py:57-61; the last duplicate wins like the dict)
 *   vertices_xy, out_xy                      float64 [n_vertices, 2]
 * Any number of handles (tables beyond 2048 handles are read through the caches instead of LDS).  Note that the reference's
 * own result depends on the BLAS kernels of its host for the weighted centroids (sgemv): this entry point follows numpy 2.2 +
 * OpenBLAS 0.3.29 on an AVX-512 host, the machine tests/golden was generated on.  VKX_ERR_DIVIDE where the reference's np.errstate(divide='raise') fires (a vertex on an integer
 * handle position that is not an exact handle hit).  _dev: device pointers, `status` int32 (zeroed by the caller)
 * receives 1 + the index of such a vertex. */
int vkx_mls_project_dev(vkx_ctx *ctx, const float *src_handles, const float *dst_handles,
                        const double *src_handles_smooth, const double *dst_handles_smooth, int n_handles,
                        const double *vertices_xy, int n_vertices, double *out_xy, int32_t *status);
int vkx_mls_project(vkx_ctx *ctx, const float *src_handles, const float *dst_handles,
                    const double *src_handles_smooth, const double *dst_handles_smooth, int n_handles,
                    const double *vertices_xy, int n_vertices, double *out_xy);

/* ---- polygon rasterisation -----------------------------------------------------------
 * cv.fillPoly(zeros((h, w), uint8), [pts], 1): PolygonInternals.np_mask element/polygon.py:70-77
 * (Bresenham LINE_8 outline + even-odd scanline spans).  pts: HOST int32 [npts, 2] as (x, y), all
 * inside the mask.  *_dev: mask is a device plane that is OR-ed into; host variant: mask is
 * overwritten with the 0/1 raster.  The raster is the one of vkx_paint_polys* and vkx_region_extend_masks_dev (one
 * definition, different stores); a polygon with more than 512 crossings on one scanline is refused (VKX_ERR_UNSUPPORTED).
 * _dev: asynchronous on the ctx stream up to 512 vertices (pts_host is consumed before the call returns); with more the
 * call waits for the overflow flag. */
int vkx_fill_poly_mask_u8_dev(vkx_ctx *ctx, const int32_t *pts_host, int npts, uint8_t *mask, int h, int w,
                              ptrdiff_t mask_stride);
int vkx_fill_poly_mask_u8(vkx_ctx *ctx, const int32_t *pts_host, int npts, uint8_t *mask, int h, int w,
                          ptrdiff_t mask_stride);

/* Ordered paint of many polygons into one label plane pair -- the label rasterisation after distortion,
 * pipeline/text_detection/page_distortion.py:163-314 (for polygon in order: polygon.fill_mask(mask) /
 * polygon.fill_score_map(score_map, value)), element/polygon.py:458-487.  Polygon i covers the cv.fillPoly
 * raster of its vertices; where polygons overlap the LAST one in the list wins, exactly like the sequential
 * fills.  Pixels inside any polygon get mask = 1 and score = values[winner]; other pixels are untouched.
 * pts_host: HOST int32 [total_pts, 2] (x, y) in plane coordinates (parts outside the plane are clipped);
 * poly_offsets_host: HOST int32 [n_polys + 1]; values_host: HOST float32 [n_polys] (required with score).
 * mask / score: either may be NULL.  A polygon with more than 64 crossings on one scanline is refused
 * (VKX_ERR_UNSUPPORTED; paint such polygons one by one through vkx_fill_poly_mask_u8 + vkx_fill_*).
 * _dev: asynchronous on the ctx stream when no polygon has more than 64 vertices (none can then exceed the crossing limit: the
 * tables travel through the context's page-locked ring); with larger polygons the call waits for the overflow flag. */
int vkx_paint_polys_dev(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                        const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                        ptrdiff_t score_stride_el, int h, int w);
int vkx_paint_polys(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                    const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                    ptrdiff_t score_stride_el, int h, int w);
/* The same paint into FRESH planes: mask / score are uninitialised device memory and every pixel of them is written (mask = 0 /
 * score = 0 outside every polygon) -- what the label rasterisation needs (it starts from np.zeros planes, page_distortion.py:201,
 * :283) without a memset dispatch per plane. */
int vkx_paint_polys_fresh_dev(vkx_ctx *ctx, const int32_t *pts_host, const int32_t *poly_offsets_host, int n_polys,
                              const float *values_host, uint8_t *mask, ptrdiff_t mask_stride, float *score,
                              ptrdiff_t score_stride_el, int h, int w);
/* ... and the label plane sets of ONE page in one call (page_distortion.py:163-314 paints four: text-line mask + height map, char
 * mask, seal-impression char mask, char height map): up to 8 sets of one plane shape, each with its own polygon list, values and
 * fresh output planes; the same pixels as n_sets vkx_paint_polys_fresh_dev calls, with one table copy and three kernels for all. */
typedef struct vkx_paint_set {
    const int32_t *pts_host;          /* HOST int32 [total_pts, 2] (x, y) */
    const int32_t *poly_offsets_host; /* HOST int32 [n_polys + 1] */
    int32_t n_polys;
    const float *values_host;         /* HOST float32 [n_polys]; required with score */
    uint8_t *mask;                    /* device [h, w] or NULL */
    ptrdiff_t mask_stride;
    float *score;                     /* device [h, w] or NULL */
    ptrdiff_t score_stride_el;
} vkx_paint_set;
int vkx_paint_poly_sets_fresh_dev(vkx_ctx *ctx, const vkx_paint_set *sets, int n_sets, int h, int w);

/* ---- the numpy Generator streams of the noise operators, drawn on the device -------------------------------------
 * photometric/noise.py:44-54 (gaussion_noise), :160-190 (speckle_noise), :100-157 (impulse_noise) draw from the
 * caller's numpy Generator (PCG64).  A job = one stream: the generator's 128-bit state and increment
 * (rng.bit_generator.state['state']) and the number of samples.  The device produces the SAME values numpy would
 * (PCG64 jump-ahead + the 256-layer ziggurat with its variable number of raw draws per sample resolved by a two-pass
 * scan), and reports how many raw 64-bit draws the call consumed, so that the caller can advance its generator
 * (state' = pcg64 jump by `draws`).  Kinds:
 *   VKX_NP_NORMAL_I16     dst int16 [n]  = np.round(rng.normal(0, scale, n)).astype(int16)
 *   VKX_NP_NORMAL_ADD_U8  dst uint8 [n]  = clip(int16(src) + the plane above, 0, 255)          (gaussion_noise, fused)
 *   VKX_NP_SPECKLE_U8     dst uint8 [n]  = uint8(clip(src + src * rng.normal(0, scale, n), 0, 255)) in float64
 *   VKX_NP_CHOICE3_U8     dst uint8 [n]  = rng.choice((0, 1, 2), n, p) as #{k : cdf[k] <= rng.random()}, cdf = cumsum(p) / sum
 *   VKX_NP_IMPULSE_U8     dst uint8 [n, cn] = src with salt (255) where the selector is 1, pepper (0) where it is 2
 *   VKX_NP_NORMAL_TILES   dst = a TILE BUFFER of vkx_np_tiles_layout(n) bytes (256-byte aligned) standing for the int16 plane of
 *                         VKX_NP_NORMAL_I16 without ever forming it: the generator works in tiles of 3072 raw draws, and a tile's
 *                         samples stay where the draw pass left them, squeezed together in the tile's slot; a table gives the
 *                         index of every tile's first sample.  vkx_chain_item.noise takes such a buffer (noise_tiled = 1): the
 *                         chain kernel looks its samples up in the slots, so gaussion_noise costs one 2-byte read per sample
 *                         instead of a placement pass (2 bytes per raw draw read, 2 bytes per sample written) plus that read.
 *                         vkx_np_tiles_expand_dev turns a buffer into the plane it stands for.
 * src / dst are dense device arrays (vkx_np_draw_batch_dev: asynchronous on the ctx stream, results_host is valid after a
 * synchronisation).  exp() / log1p() of the device differ from glibc's in the last bits: a decision or an
 * emitted integer that could depend on them sets VKX_NP_AMBIGUOUS in the job's result (the caller then redraws that plane
 * with numpy itself; expected < 1e-6 per 2048^2 plane); VKX_NP_SHORT = the provisioned raw draws did not yield n samples
 * (same remedy; never observed). */
#define VKX_NP_NORMAL_I16 0
#define VKX_NP_NORMAL_ADD_U8 1
#define VKX_NP_SPECKLE_U8 2
#define VKX_NP_CHOICE3_U8 3
#define VKX_NP_IMPULSE_U8 4
#define VKX_NP_NORMAL_TILES 5
#define VKX_NP_DEBUG_WIDE_MARGIN 0x100 /* or-ed into kind: every wedge test counts as ambiguous (exercises the fallback in tests) */
#define VKX_NP_AMBIGUOUS 1u
#define VKX_NP_SHORT 2u
typedef struct vkx_np_job {
    uint64_t state[2];   /* PCG64 state, low / high word */
    uint64_t inc[2];     /* PCG64 increment, low / high word */
    int64_t n;           /* samples (normal kinds) or elements (uniform kinds) */
    int32_t kind, cn;
    double scale;        /* std of the normal kinds */
    double cdf[3];       /* uniform kinds */
    const void *src;     /* device */
    void *dst;           /* device */
} vkx_np_job;
typedef struct vkx_np_result {
    unsigned long long draws;    /* raw 64-bit draws consumed */
    unsigned long long samples;  /* samples the provisioned draws yielded (>= n unless VKX_NP_SHORT) */
    uint32_t flags, reserved;
} vkx_np_result;
int vkx_np_draw_batch_dev(vkx_ctx *ctx, const vkx_np_job *jobs_host, int n_jobs, vkx_np_result *results_host);
/* Tile buffer of a VKX_NP_NORMAL_TILES job of n samples: `bytes` in all; a 16-byte header (uint32 tiles, uint32 slot elements,
 * uint64 samples the tiles hold), at table_offset [n_tiles + 1] x (uint32 index of the tile's first sample, uint32 first valid
 * element of its slot), at slots_offset n_tiles slots of slot_elems int16.  Sample i of the plane, with
 * table[t].first <= i < table[t + 1].first, is slot t's element table[t].skip + i - table[t].first; samples i + 1 .. i + 3 follow
 * it in the same slot (a slot ends with the first three samples of its successor).  Any output pointer may be NULL. */
int vkx_np_tiles_layout(int64_t n, int64_t *n_tiles, int64_t *slot_elems, int64_t *table_offset, int64_t *slots_offset, int64_t *bytes);
/* Debug: 1 when the draw pass parks the samples of an int16 job with this scale (and location; the jobs above have 0) as bytes,
 * i.e. when 3.6541528853610088 |scale| + |loc| <= 127, the largest integer a ziggurat fast accept can become; 0 otherwise.  The
 * samples are the same either way; a launch parks bytes when all its jobs qualify.  No device needed. */
int vkx_np_parks_as_bytes(double scale, double loc);
/* dst int16 [n] (device, 8-byte aligned) = the plane a finished tile buffer stands for; asynchronous on the ctx stream */
int vkx_np_tiles_expand_dev(vkx_ctx *ctx, const void *tiles, int64_t n, int16_t *dst);
/* Debug: est[i] (device, float64) = the float32-logarithm estimate of -log(1 - u), u = (draws[i] >> 11) * 2^-53, from which the integer
 * kinds decide a ziggurat tail pass; *eps (host, may be NULL) = the absolute error the kernels assume of it.  Asynchronous on the ctx
 * stream.  The kernels take the float64 log1p wherever that error could change a decision or an emitted integer. */
int vkx_np_tail_log_est_dev(vkx_ctx *ctx, const uint64_t *draws, int64_t n, double *est, double *eps);
/* one job whose src / dst are HOST arrays; synchronous */
int vkx_np_draw(vkx_ctx *ctx, const vkx_np_job *job, vkx_np_result *result_host);

/* rng.poisson(lam) with lam = the bytes of a uint8 array (vkit poisson_noise, photometric/noise.py:81-90: `rng.poisson(mat as float32)`
 * + clip to uint8), value for value numpy 2.2.6's random_poisson per element in C order (distributions.c: nothing for lam 0, the
 * multiplication method below 10, PTRS from 10 up), drawn on the device from the PCG64 stream (state, inc) although every element takes
 * a data-dependent number of draws: windows of candidate stream positions per block of 32 elements, resolved superblock by superblock
 * (vkit_amd/csrc/poisson.hip).  dst uint8 [n] = min(sample, 255); *consumed_host = the raw 64-bit draws numpy would have made.
 * *flags_host != 0: the result is NOT to be used and the stream not to be moved (the caller draws with numpy on the host): a PTRS
 * comparison fell within 2e-13 of equality (device log vs glibc log), a start left its 6-sigma window, or the stream would need more than 2^29 raw draws.
 * Synchronous.  _dev: device arrays, src 16-byte aligned. */
#define VKX_NP_POISSON_AMBIGUOUS 1u
#define VKX_NP_POISSON_TABLE 2u     /* not raised any more: k + 1 beyond the loggam table takes random_loggam with the device log */
#define VKX_NP_POISSON_WINDOW 4u
#define VKX_NP_POISSON_MISMATCH 8u
#define VKX_NP_POISSON_DRAWS 16u
#define VKX_NP_POISSON_SIZE 32u   /* the stream would take more than 2^29 raw draws (4 GB of scratch) */
int vkx_np_poisson_u8_dev(vkx_ctx *ctx, const uint64_t *state, const uint64_t *inc, const uint8_t *src, long long n, uint8_t *dst,
                          long long *consumed_host, unsigned *flags_host);
int vkx_np_poisson_u8(vkx_ctx *ctx, const uint64_t *state, const uint64_t *inc, const uint8_t *src_host, long long n, uint8_t *dst_host,
                      long long *consumed_host, unsigned *flags_host);
/* out[x - 1] = numpy's random_loggam(x), x = 1 .. n, as the library tabulates it on the host (tests compare it with libnpyrandom.a) */
int vkx_np_poisson_loggam_table(double *out, int n);

/* The fog density field of `fog` (reference photometric/effect.py:89-216) on the device: the diamond-square lattice of
 * generate_diamond_square_mask -- (2^levels + 1)^2 float32, field 4-byte aligned device memory whose four corners the caller drew
 * (corners_host: [0, 0], [0, -1], [-1, -1], [-1, 0]) -- filled level by level with numpy's float32 / float64 roundings from the PCG64
 * stream (state, inc) positioned AFTER the corner draws; noise_weight_host[l] = roughness ** l as Python computes it.
 * *consumed_host = the raw draws taken (the caller moves its generator, then draws the crop offsets).  Asynchronous on the ctx stream.
 * vkx_fog_stretch_f32_dev: mask float32 [h, w] = the crop (up, left) stretched like the reference: x - min, / max, * float32(span),
 * + float32(lo).  (vkit_amd/csrc/fog.hip) */
int vkx_fog_field_f32_dev(vkx_ctx *ctx, const uint64_t *state, const uint64_t *inc, int levels, const double *noise_weight_host,
                          const float *corners_host, float *field, long long *consumed_host);
int vkx_fog_stretch_f32_dev(vkx_ctx *ctx, const float *field, int size, int up, int left, int h, int w, double span, double lo, float *mask);

/* glass_blur's shuffle planes (reference photometric/blur.py:204-250) kept on the device: pos_y / pos_x int32 [h, w] dense planes, the
 * operands of vkx_gather_u8_dev.  vkx_glass_init_dev: the identity (and the context's scratch for the rounds).  vkx_glass_round_dev: one
 * round of swaps -- centres at rows r0 + i pitch (i < n_rows), columns c0 + j pitch (j < n_cols); centre k = i n_cols + j exchanges its
 * entry with the one at clip(its current source position + (jump_y[k], jump_x[k])) with numpy's semantics of
 * `pos[centres], pos[to] = pos[to], pos[centres]` (right sides first, the last centre in C order wins a shared `to`).  The jumps are host
 * arrays (the caller's rng.integers draws); synchronous on return.  (vkit_amd/csrc/fog.hip) */
int vkx_glass_init_dev(vkx_ctx *ctx, int32_t *pos_y, int32_t *pos_x, int h, int w);
int vkx_glass_round_dev(vkx_ctx *ctx, int32_t *pos_y, int32_t *pos_x, int h, int w, int r0, int c0, int pitch, int n_rows, int n_cols,
                        const int32_t *jump_y_host, const int32_t *jump_x_host);

/* ---- throughput-mode noise plane ---------------------------------------------------------------
 * gaussion_noise (photometric/noise.py:44-54) adds np.round(rng.normal(0, std, shape)) drawn from the caller's numpy
 * Generator; the parity path takes that int16 plane from the caller (vkx_add_noise_i16, vkx_chain_item.noise).
 * vkx_noise_normal_i16 draws a plane with the same DISTRIBUTION on the device -- not the same values, which are a
 * function of numpy's bit stream: sample s of the flat C-order plane takes the (s & 3)-th 16-bit uniform of the
 * Philox2x32-10 block with counter (s >> 2, seed >> 32) and key = seed low word, and maps it through a 65536-entry
 * inverse-CDF table of round(N(0, std)) (vkx_noise_normal_table builds that table on the host, for checks).
 * Separately labelled: a caller opts in.
 * dst: int16 [h, w, cn], cn in 1..4; _dev: device plane (8-byte aligned when dense: stride_el == w * cn), asynchronous;
 * host variant: host plane, synchronous. */
int vkx_noise_normal_table(double std, int16_t *table_host /* [65536] */);
int vkx_noise_normal_i16_dev(vkx_ctx *ctx, int16_t *dst, ptrdiff_t stride_el, int h, int w, int cn, double std, uint64_t seed);
/* the planes of a batch that share `std` in one launch (each with its own seed): the table is staged once per workgroup */
typedef struct vkx_noise_plane {
    int16_t *dst;          /* device */
    ptrdiff_t stride_el;
    int h, w, cn, reserved;
    uint64_t seed;
} vkx_noise_plane;
int vkx_noise_normal_i16_batch_dev(vkx_ctx *ctx, const vkx_noise_plane *planes_host, int n_planes, double std);
int vkx_noise_normal_i16(vkx_ctx *ctx, int16_t *dst, ptrdiff_t stride_el, int h, int w, int cn, double std, uint64_t seed);

/* ---- batched geometric + photometric chain (device resident) ---------------------------
 * RandomDistortion's geometric stage followed by photometric members on one page image
 * (mechanism/distortion_policy/random_distortion.py:190-203 applied through
 * Distortion.distort, mechanism/distortion/interface.py:824-912), for a ragged batch of
 * independent images: image-grid remap -> gaussian_blur -> color_shift -> gaussion_noise -> line_streak
 * (photometric/streak.py:56-99); stages with a disabled parameter are skipped.
 * `items` is a HOST array; every pointer inside is a DEVICE pointer. */
typedef struct vkx_chain_item {
    const uint8_t *src;            /* uint8 [sh, sw, 3] */
    uint8_t *dst;                  /* uint8 [dh, dw, 3] */
    ptrdiff_t src_stride, dst_stride;
    int32_t sh, sw, dh, dw;
    const int32_t *src_vertices;   /* int32 [rows, cols, 2] (x, y) */
    const int32_t *dst_vertices;
    int32_t rows, cols;
    const int16_t *noise;          /* optional int16 [dh, dw, 3]; NULL = no noise stage.  noise_tiled: the tile buffer of a
                                      VKX_NP_NORMAL_TILES job of dh * dw * 3 samples instead (noise_stride_el unused) */
    ptrdiff_t noise_stride_el;
    double blur_sigma;
    int32_t blur_ksize;            /* <= 1 = no blur stage */
    int32_t hue_delta;
    int32_t hue_enabled;           /* 0 = no color_shift stage */
    int32_t streak_enabled;        /* 0 = no line_streak stage */
    int32_t streak_thickness, streak_gap, streak_dash_thickness, streak_dash_gap;
    int32_t streak_enable_vert, streak_enable_hori;
    uint8_t streak_color[4];
    int32_t noise_tiled;           /* 0: `noise` is a plane */
    double streak_alpha;           /* in [0, 1] */
} vkx_chain_item;
int vkx_chain_rgb_batch_dev(vkx_ctx *ctx, const vkx_chain_item *items, int n_items);
/* The numpy streams of a batch's gaussion_noise members and its chain in ONE call: jobs = VKX_NP_NORMAL_TILES jobs, each drawing the
 * tile buffer that is the `noise` (noise_tiled = 1) of one item, in item order.  Same results as vkx_np_draw_batch_dev(jobs) followed
 * by vkx_chain_rgb_batch_dev(items); the library cuts the batch into chunks of images and runs the microsecond kernels of either
 * call (carry resolution, tile tables, cell setup, noise row records: eight launches of a few workgroups) on the context's two other
 * streams, under the draw pass of the next chunk or the pixel kernel of the first one (vkit_amd/csrc/chain.hip).  Jobs of another
 * kind, or items the fused kernel declines, make it exactly the two calls.  Asynchronous on the ctx stream. */
int vkx_chain_rgb_batch_np_dev(vkx_ctx *ctx, const vkx_chain_item *items, int n_items, const vkx_np_job *jobs_host, int n_jobs,
                               vkx_np_result *results_host);
/* The cell setup of a chain call (one lane per lattice cell: homographies, edge tables, tile bins) reads nothing but the vertex
 * lattices and runs on a side stream of the context.  By default it starts after everything queued on the ctx stream before the
 * chain call.  A caller whose lattices are complete earlier says so: this call marks the current point of the ctx stream, and the
 * setup of the NEXT chain call waits for that point only (e.g. it then runs under a page composite queued between the mark and the
 * chain call).  One chain call per mark: a mark never outlives the lattices it spoke of. */
int vkx_chain_lattices_ready(vkx_ctx *ctx);

/* ---- camera-model states built on the device ------------------------------------------------------------------------
 * The state of camera_plane_only / camera_cubic_curve (mechanism/distortion/geometric/camera.py:58-265, 324-423: CameraModel,
 * the 2-D -> 3-D strategies, cv.Rodrigues / cv.projectPoints; grid_rendering/grid_creator.py:44-115: source lattice, projection,
 * shift by the rounded minimum; element/point.py:31-47: rounding) for a BATCH of configs: the dozen scalars of a state on the host
 * in C (vkx_camera_model_host: float32 / float64 exactly where numpy computes in them, libm's sin / cos / tan like Python's math
 * module), the per-vertex work on the device, one workgroup per state.  The vertex lattices come out bit for bit the host
 * operator's (tests/golden/camera_states.npz).  vkit_amd/csrc/camera.hip */
#define VKX_CAMERA_PLANE_ONLY 0
#define VKX_CAMERA_CUBIC_CURVE 1
typedef struct vkx_camera_config {
    int32_t kind, height, width, grid_size;
    double rotation_unit_vec[3];
    double rotation_theta;
    double focal_length, camera_distance;   /* 0 = not given: completed from the shape like the reference */
    double principal_point[3];
    int32_t principal_point_len;            /* 0 = not given; 2 or 3 */
    int32_t reserved;
    double curve_alpha, curve_beta, curve_direction, curve_scale;     /* VKX_CAMERA_CUBIC_CURVE */
} vkx_camera_config;
typedef struct vkx_camera_model {           /* what the per-vertex kernel consumes; exposed for the parity tests */
    double R[9], t[3];                      /* float64 Rodrigues matrix of the float32 rotation vector; float32 translation as double */
    double fx, fy, cx, cy;
    float a0, a1, along_min, along_range;   /* cubic curve: first row of the float32 direction matrix, extent of the page along it */
    double poly[4], curve_scale;
    int32_t rows, cols;                     /* lattice shape */
    int32_t points_f32, reserved;           /* the projected points take float32 (plane only: float32 3-D points) */
} vkx_camera_model;
#define VKX_GRID_STATE_NAN 1u               /* a projected vertex is NaN (the reference raises ValueError in Point's round()) */
#define VKX_GRID_STATE_INF 2u               /* ... infinite (OverflowError) */
#define VKX_GRID_STATE_RANGE 4u             /* the lattice leaves int32 */
#define VKX_GRID_STATE_DIVIDE 8u            /* similarity_mls: a vertex on an integer handle position (the reference raises FloatingPointError) */
typedef struct vkx_grid_state {
    int32_t rows, cols, dh, dw;             /* lattice shape; result shape = extent of the destination lattice */
    int32_t shift_y, shift_x;               /* DistortionStateImageGridBased.shift_amount_* */
    uint32_t flags, reserved;
} vkx_grid_state;
int vkx_camera_model_host(const vkx_camera_config *config, vkx_camera_model *out);
/* src_vertices / dst_vertices: HOST arrays of n DEVICE pointers to int32 [rows, cols, 2] (x, y) lattices (rows / cols of a config:
 * vkx_camera_model_host).  stream: VKX_STREAM_*: on which of the context's streams the states are built -- a side stream builds
 * the states of the next batch while the compute stream still runs the current one.  states_host (page-locked memory for an
 * asynchronous copy) is valid after vkx_ctx_sync_stream(ctx, stream).  The chain calls that follow start their cell setup after
 * this call's kernel (it records the lattices-ready point of vkx_chain_lattices_ready). */
int vkx_camera_states_dev(vkx_ctx *ctx, const vkx_camera_config *configs_host, int n, int32_t *const *src_vertices,
                          int32_t *const *dst_vertices, vkx_grid_state *states_host, int stream);

/* SimilarityMlsState (geometric/mls.py:140-157; SimilarityMlsPointProjector.project_point :38-135 per lattice vertex, then
 * grid_rendering/grid_creator.py:44-115 with resize_as_src = False, the operator's default) for a BATCH of configs: handle tables are
 * HOST arrays -- float32 [n, 2] integer positions (PointTuple.to_smooth_np_array) and float64 [n, 2] smooth positions of the source and
 * destination handles --, the lattices DEVICE buffers as for vkx_camera_states_dev, to which everything else said there applies.
 * (vkit_amd/csrc/mls.hip) */
typedef struct vkx_mls_config {
    int32_t height, width, grid_size, n_handles;
    const float *src_handles, *dst_handles;
    const double *src_handles_smooth, *dst_handles_smooth;
} vkx_mls_config;
int vkx_mls_states_dev(vkx_ctx *ctx, const vkx_mls_config *configs_host, int n, int32_t *const *src_vertices,
                       int32_t *const *dst_vertices, vkx_grid_state *states_host, int stream);

/* ---- page cropping ---------------------------------------------------------------------
 * PageCroppingStep (pipeline/text_detection/page_cropping.py:243-290) and Cropper (mechanism/cropper.py:333-376) on
 * device-resident planes.  Every plane is DENSE (rows follow each other without gaps; the pitch is width x channels), so
 * none of these entry points takes a stride.  The window of one crop, in page coordinates: the part of the page a crop
 * of crop_size = core_size + 2 pad_size covers (Cropper.original_box, clipped to the page by construction) and where it
 * lands in the crop (target_box.up / .left, mechanism/cropper.py:106-160).  The core of the crop is the square
 * [pad_size, pad_size + core_size) of crop coordinates (target_core_box, ibid.). */
typedef struct vkx_crop_window {
    int32_t up, left, height, width;   /* original_box: inside the page, height and width >= 1 */
    int32_t target_up, target_left;    /* target_box origin: the window lies inside the crop */
} vkx_crop_window;

/* The counts behind PageCroppingStep's accept / reject loop for a batch of candidate windows, in one launch:
 *   item 0: pixels of the page image with any channel > 0 (num_samples estimate, page_cropping.py:254-262), counted when
 *           `image` is not NULL;
 *   item 1 + i: slot 0 = char_mask pixels > 0 inside the core of window i (text ratio, page_cropping.py:142-146),
 *               slot 1 = active_mask pixels > 0 inside window i (active ratio, page_cropping.py:148-152).
 * Padding adds nothing to either count, so these equal the reference's counts on the padded crop.  The result is per
 * workgroup partial sums: partials = int64 [1 + n_windows][n_parts][2] in DEVICE memory, the caller adds up the n_parts
 * entries of every (item, slot) -- exact integers, no atomics, no clearing pass.  `windows_host` is a HOST table.
 * image h x w x cn (cn 1, 3 or 4), the two masks uint8 h x w, all device, dense. */
int vkx_crop_count_dev(vkx_ctx *ctx, const uint8_t *image, int h, int w, int cn, const uint8_t *active_mask,
                       const uint8_t *char_mask, int core_size, int pad_size, const vkx_crop_window *windows_host,
                       int n_windows, int n_parts, int64_t *partials);

/* One plane of one crop for vkx_crop_planes_dev: Cropper.crop_image / crop_mask / crop_score_map (mechanism/cropper.py:
 * 333-376) -- the window copied, the rest of the crop filled -- and, for a core-only plane, the INTER_AREA shrink by an
 * integer factor that PageCroppingStep applies to its labels (page_cropping.py:154-230: Mask.to_resized_mask's
 * x255 -> cv.resize -> > 0 for masks, ScoreMap.to_resized_score_map with its [0, 1] clip for probability maps).  The
 * shrink is the arithmetic of vkx_resize_u8 / vkx_resize_f32's integer-factor INTER_AREA path, bit for bit. */
typedef struct vkx_crop_plane {
    const void *src;      /* device, the page plane h x w x cn, dense */
    void *dst;            /* device, crop_size^2 (core_only 0) or core_size^2 (core_only 1) x cn, dense */
    void *dst_down;       /* device, (core_size / factor)^2, or NULL; core-only planes only */
    int32_t cn;           /* uint8: 1, 3 or 4; float32: 1 */
    int32_t is_f32;       /* 0 uint8, 1 float32 */
    int32_t core_only;    /* 1: only the core of the crop (crop_mask / crop_score_map with core_only=True) */
    int32_t is_mask;      /* uint8 shrink as Mask.to_resized_mask (on (v > 0) * 255, then > 0); 0: plain INTER_AREA */
    int32_t clip;         /* float32 shrink clipped to [0, 1] (ScoreMap.is_prob) */
    int32_t fill;         /* the value of the padding in every channel: 0 .. 255 for uint8 planes, 0 for float32 */
    int32_t window;       /* index into the window table */
} vkx_crop_plane;
/* All planes of all crops in one launch.  `windows_host` and `planes_host` are HOST tables; factor 0 = no shrink, else
 * it divides core_size and pad_size.  Refused (VKX_ERR_INVALID, nothing written) for a NULL pointer, a window outside the
 * page or the crop, a channel count other than 1 / 3 / 4, a factor that does not divide and a destination overlapping a
 * source. */
int vkx_crop_planes_dev(vkx_ctx *ctx, int h, int w, int core_size, int pad_size, int factor, const vkx_crop_window *windows_host,
                        int n_windows, const vkx_crop_plane *planes_host, int n_planes);

/* ---- the combiner image engine (engine/image/combiner.py:178-333, ImageCombinerEngine.synthesize_image) -----------------
 * Writes the whole page dst = uint8 [h, w, 3] (device, dense) in one launch from texture tiles:
 *   mosaic = zeros, then every tile in table order: mosaic[up : down + 1, left : right + 1] = the upper left
 *            (down + 1 - up) x (right + 1 - left) corner of its source image (combiner.py:286-291); a pixel no tile covers
 *            is 0, a pixel two tiles cover takes the later one;
 *   edge   = union over the tiles of the four bands of fill_np_edge_mask (combiner.py:146-176): rows [up - half, up + half]
 *            and [down - half, down + half] over columns left .. right, columns [left - half, left + half] and
 *            [right - half, right + half] over rows up .. down, clipped to the page;
 *   dst    = edge ? cv.GaussianBlur(mosaic, (ksize, ksize), sigma) : mosaic (combiner.py:326-331), the blur with the
 *            arithmetic of vkx_gaussian_blur_u8_dev (8.8 fixed point, BORDER_REFLECT_101) on the UNBLURRED mosaic.
 * The reference passes half = gaussian_blur_kernel_size / 2 + 1 and sigma = half / 3.  `tiles_host` and `sources_host` are
 * HOST tables; a source's image is a DEVICE pointer.  Asynchronous on the context's stream.  Refused (VKX_ERR_INVALID,
 * nothing written) for a NULL pointer, h or w outside 0 .. 2^19 or h * w >= 2^29 (an empty page writes nothing), ksize even,
 * below 1 or above 15 (the LDS window of a 64 x 16 block holds a halo of 7), half outside 0 .. 64, sigma not finite or
 * <= 0, a tile outside the page or larger than its source, a source index out of range, a source without pixels, a
 * destination overlapping a source, and a table whose tiles meet more than 2^26 (64 x 16 block, tile) pairs in all. */
typedef struct vkx_combine_tile {
    int32_t up, down, left, right;     /* inclusive, inside the page */
    int32_t source;                    /* index into the source table */
} vkx_combine_tile;
typedef struct vkx_combine_source {
    const uint8_t *image;              /* device, uint8 [height, width, 3], dense */
    int32_t height, width;
} vkx_combine_source;
int vkx_image_combine_u8c3_dev(vkx_ctx *ctx, const vkx_combine_tile *tiles_host, int n_tiles,
                               const vkx_combine_source *sources_host, int n_sources, int ksize, int half, double sigma,
                               uint8_t *dst, int h, int w);

/* ---- the external_ellipse char-mask engine (engine/char_mask/external_ellipse.py:104-220) ------------------------------
 * Per char (4 points, smooth float64 (x, y)) and internal side length L (1 .. 2048): R = ceil(L / sqrt 2), E = 2 R + 1, the
 * template build_np_distance(R) <= R (engine/char_heatmap/default.py:30-40); H1 = getPerspectiveTransform(char square
 * [pad, pad + L - 1]^2, pad = (E - L) // 2 -> the polygon's float32 self-relative points) with the project's DECOMP_SVD
 * definition (closed form, Jacobi SVD for degenerate quads); the 4 corners of [0, E - 1]^2 through H1 as affine_np_points
 * computes them (numpy's matmul: fma(h2, 1, fma(h1, y, h0 x)), then / w); their min x / y subtracted, cast to float32;
 * H2 = getPerspectiveTransform(external corners -> those); warpPerspective(template, H2, (ceil(x max), ceil(y max)))
 * INTER_LINEAR, BORDER_CONSTANT 0 (a zero side: the template's size, as cv2); placed at round(min smooth y / x + offset)
 * (halves to even) and trimmed against the page or the char's bounding box (:156-200).  A sample != 0 covers its pixel:
 * mask = 1 there (:218), and score = the value of the LAST char of the set covering the pixel (PageDistortionStep's height
 * map, pipeline/text_detection/page_distortion.py:276-287); every other pixel of both planes is 0.  char_masks, when given,
 * receives every char's trimmed warped template (the reference's char_masks[i].mat), row-major, one after the other in
 * char order.
 * Status per char in boxes_host [n_chars, 5] = (up, down, left, right, status): 0 placed (the trimmed box); 1 the box and
 * the trimmed template differ in shape (the reference raises RuntimeError: the disc lies outside the page / box); 2 an
 * empty box (AssertionError in Box.extract_np_array: the quad collapses); 3 a NaN size (ValueError in math.ceil); 4 an
 * infinite or larger than 2^30 size or position (OverflowError).  When any char has a non-zero status the call returns
 * VKX_ERR_CHAR_MASK after filling boxes_host and writes no plane.
 * One call: the sets of one page (up to 8), three launches and one synchronisation (the boxes).  Planes are dense.  Refused
 * (VKX_ERR_INVALID, nothing written) before any launch for L outside 1 .. 2048, a polygon without exactly 4 points, a
 * non-finite point, a bounding box outside the page, a score plane without values and overlapping output planes; a
 * char_masks_cap below the packed size is refused after the boxes are known (boxes_host filled, no plane written). */
typedef struct vkx_char_set {
    const double *pts_host;           /* HOST float64 [total_pts, 2] (x, y) */
    const int32_t *poly_offsets_host; /* HOST int32 [n_chars + 1]: 4 points each */
    int32_t n_chars;
    const int32_t *bounds_host;       /* HOST int32 [n_chars, 4] (up, down, left, right) inside the page, or NULL: the page */
    const float *values_host;         /* HOST float32 [n_chars]; required with score */
    uint8_t *mask;                    /* [h, w] or NULL */
    float *score;                     /* [h, w] or NULL */
    uint8_t *char_masks;              /* the packed per-char masks, or NULL */
    int64_t char_masks_cap;           /* bytes of char_masks */
    int32_t *boxes_host;              /* HOST int32 [n_chars, 5] out */
} vkx_char_set;
/* _dev: mask / score / char_masks in device memory.  The host form: in host memory, returns after the copies back. */
int vkx_char_mask_ellipse_sets_fresh_dev(vkx_ctx *ctx, int internal_side_length, const vkx_char_set *sets, int n_sets, int h, int w);
int vkx_char_mask_ellipse_sets_fresh(vkx_ctx *ctx, int internal_side_length, const vkx_char_set *sets, int n_sets, int h, int w);

/* ---- the default char-heatmap engine (engine/char_heatmap/default.py:93-180) ---------------------------------------------
 * Per char (4 points, smooth float64 (x, y)), in list order: H = getPerspectiveTransform(template corners (0, 0), (2r, 0),
 * (2r, 2r), (0, 2r) -> the polygon's float32 self-relative integer points round(smooth) - min) with the project's DECOMP_SVD
 * definition; warpPerspective(template, H, (bbox.width, bbox.height)) float32, INTER_LINEAR, BORDER_CONSTANT 0; keep-max into
 * score_map_max (0 at first) and keep-min into score_map_min (1 at first) at the pixels of the char's cv.fillPoly raster
 * (Polygon.internals.np_mask).  Then per page pixel: overlapped = covered by the rasters of 2 or more chars; neutralized =
 * overlapped && !(max >= preserving_score_min); delta = clip(max - min, 0, 1); nscore = neutralized ? delta : max;
 * score = weight_max * max + weight_neutralized * nscore, each product and the sum rounded to float32.
 * One call: one page, three launches, no synchronisation (_dev).  Planes are dense.  Refused (VKX_ERR_INVALID, nothing
 * written) before any launch for a NULL pointer, a radius outside 1 .. 1024, h or w outside 1 .. 2^24 - 1 or h * w >= 2^31,
 * n_chars outside 0 .. 2^24 - 1, a non-finite point, a char box outside the page, a debug record with a NULL plane and
 * output planes that overlap one another. */
typedef struct vkx_char_heatmap_config {
    int32_t radius;                  /* r: the template is (2r + 1) x (2r + 1) */
    int32_t reserved;                /* 0 */
    const float *template_host;      /* HOST float32 [2r + 1][2r + 1]: build_np_distance's Gaussian map, values in [0, 1] */
    float preserving_score_min;      /* float32(gaussian_map_preserving_score_min) */
    float weight_max;                /* float32(1 - weight_neutralized_score_map), the difference taken in double */
    float weight_neutralized;        /* float32(weight_neutralized_score_map) */
    float reserved2;                 /* 0 */
} vkx_char_heatmap_config;
typedef struct vkx_char_heatmap_debug {   /* CharHeatmapDefaultDebug: all six planes [h, w] */
    float *score_map_max;
    float *score_map_min;
    uint8_t *char_overlapped_mask;
    float *char_neutralized_score_map;    /* delta */
    uint8_t *neutralized_mask;
    float *neutralized_score_map;
} vkx_char_heatmap_debug;
/* _dev: score and the debug planes in device memory; the host form: in host memory, returns after the copies back.
 * quads_host: HOST float64 [n_chars][4][2] (x, y).  debug: NULL or a record of six planes. */
int vkx_char_heatmap_fresh_dev(vkx_ctx *ctx, const vkx_char_heatmap_config *config, const double *quads_host, int n_chars,
                               int h, int w, float *score, const vkx_char_heatmap_debug *debug);
int vkx_char_heatmap_fresh(vkx_ctx *ctx, const vkx_char_heatmap_config *config, const double *quads_host, int n_chars,
                           int h, int w, float *score, const vkx_char_heatmap_debug *debug);

/* ---- PageTextRegionLabelStep (pipeline/text_detection/page_text_region_label.py) ----------------------------------------
 * vkx_region_label_deviate_dev replaces the deviate-candidate loop of generate_page_char_regression_labels (:498-575): per
 * char g < n_chars (4 points, smooth float64 (x, y)) and per candidate j < m, with the box (up, left, bh, bw) of the rounded
 * points (Polygon.bounding_box) and H = getPerspectiveTransform((0, 0), (bw - 1, 0), (bw - 1, bh - 1), (0, bh - 1) -> the
 * float32 self-relative integer points) with the project's DECOMP_SVD definition, the drawn point (x, y) maps as affine_points
 * does (float64 H times the float32 (x, y, 1) in numpy's matmul order, a single column (m == 1) in its matrix-vector
 * order, then the two divisions) to (px, py); out = (up + py,
 * left + px), their rint, a status (0 in the page, 1 dropped: the last of m > 2 points equals the first as integers, as
 * PointTuple.from_np_array drops it; 2 outside [0, h) x [0, w); 3 non-finite) and, for status 0, the nearest-centre class
 * that replaces KDTree(centres).query (:468, :541): 0 the char's own centre strictly nearest, 1 another strictly nearer, 2 a
 * tie at the minimum (the host resolves it).  Squared distances of integer points, exact.  One launch, no synchronisation.
 * Refused (VKX_ERR_INVALID, nothing launched) for a NULL pointer, n_centres outside 1 .. 2^24 - 1, n_chars outside
 * 1 .. n_centres, m outside 1 .. 4096, h or w outside 1 .. 32768, a centre or a point outside +-2^30, a non-finite point, a
 * box narrower or lower than 3 and a draw outside [1, bw - 2] x [1, bh - 2]. */
typedef struct vkx_region_label_deviate_out {
    double y, x;          /* the smooth page point */
    int32_t iy, ix;       /* rint(y), rint(x) (status 0) */
    int32_t status;       /* 0 in the page, 1 dropped, 2 outside the page, 3 non-finite */
    int32_t cls;          /* status 0: 0 keep, 1 drop, 2 tie */
} vkx_region_label_deviate_out;
/* quads_host: HOST float64 [n_chars][4][2] (x, y); centres_host: HOST int32 [n_centres][2] (x, y), char g's centre at g;
 * draws_host: HOST int32 [n_chars][m][2] (x, y); out: DEVICE [n_chars * m]. */
int vkx_region_label_deviate_dev(vkx_ctx *ctx, const double *quads_host, const int32_t *centres_host, int n_centres,
                                 int n_chars, const int32_t *draws_host, int m, int h, int w, vkx_region_label_deviate_out *out);
/* vkx_region_label_planes_dev replaces generate_page_char_bounding_box_mask (:578-592) and the inactive fills of
 * generate_page_char_mask (:406) and generate_page_char_height_score_map (:439): box_mask = 1 inside any of the boxes
 * (up, down, left, right), 0 elsewhere; char_mask = 0 and char_height = 0.0f where active_mask == 0.  Dense device planes
 * [h, w].  One launch, no synchronisation.  Refused for a NULL pointer, n_boxes outside 0 .. 2^24 - 1, h or w outside
 * 1 .. 32768, a box not inside the page, planes that overlap one another, and more than 2^28 (box, 32 x 32 tile) pairs over
 * the tiles that no box covers whole ("too many (box, tile) pairs"). */
int vkx_region_label_planes_dev(vkx_ctx *ctx, const int32_t *boxes_host, int n_boxes, int h, int w, const uint8_t *active_mask,
                                uint8_t *char_mask, float *char_height, uint8_t *box_mask);

/* ---- PageTextRegionCroppingStep (pipeline/text_detection/page_text_region_cropping.py) ----------------------------------
 * vkx_region_crop_select_dev replaces the two STRtree queries and the preserved-char filter of one attempt (:160-187), for
 * every candidate window of a page at once.  Per window (up, down, left, right) -- an original_core_box, which may reach
 * outside the page --: a centroid label (x, y, char_idx) is kept when left <= x <= right and up <= y <= down (closed bounds:
 * a shapely box intersects a point on its edge); a deviate label is kept when it passes the same test and its char_idx is
 * the char_idx of a kept centroid label of that window.  counts[window] = (kept centroid labels, kept deviate labels);
 * row `window` of each index table holds the kept label indices in ascending order (the reference walks sorted(query(...)))
 * in its first count entries, the rest of the row is unspecified.  Integer compares only.  Dense tables, no pitch.  One
 * launch, no synchronisation.  While every char_idx is below 262 144 the call keeps nothing but the staged tables on the
 * context; beyond that it reserves up to 64 MB of context scratch for bitmaps, kept until the context is destroyed.
 * Refused (VKX_ERR_INVALID, nothing launched) for a NULL pointer (a table or an index table of
 * zero labels may be NULL), n_windows outside 1 .. 4096, a label count outside 0 .. 2^24 - 1, a char_idx outside
 * 0 .. 2^24 - 1, a box with down < up or right < left and outputs that overlap one another.
 * windows_host: HOST int32 [n_windows][4]; centroid_host / deviate_host: HOST int32 [n][3]; counts: DEVICE int32
 * [n_windows][2]; centroid_rows / deviate_rows: DEVICE int32 [n_windows][n_centroid] / [n_windows][n_deviate]. */
int vkx_region_crop_select_dev(vkx_ctx *ctx, const int32_t *windows_host, int n_windows, const int32_t *centroid_host,
                               int n_centroid, const int32_t *deviate_host, int n_deviate, int32_t *counts,
                               int32_t *centroid_rows, int32_t *deviate_rows);

/* ---- the pixel half of PageTextRegionStep (pipeline/text_detection/page_text_region.py) ---------------------------------
 * Four batched entry points, each ONE launch for all text regions of a page and no synchronisation; their per-region records
 * are HOST tables (a fifth, vkx_region_extend_masks_dev below, builds the masks they start from).  A record addresses its source planes by device pointer and row step (bytes from a row to the next, at
 * least one row, unused with a single row: the pitch contract of this header), so a source may be a rectangle inside a
 * page plane or a plane of its own; what a call writes is dense and lies at a byte offset of one packed buffer `dst` of
 * `dst_bytes` bytes.  Refused (VKX_ERR_INVALID, nothing launched): a NULL pointer, a count outside 1 .. 4096 (0 .. 4096 for
 * the stack), a side outside 1 .. 32767, a row step shorter than a row or negative, a destination outside `dst`,
 * destinations that overlap one another and a source plane that overlaps `dst`.  A pair writes its image, its mask or
 * both: a negative dst_image_off / dst_mask_off leaves that plane out, and its source pointer is then not read (the
 * reference trims and resizes image and mask by separate calls, whose shapes can differ: Image.to_cropped_image takes
 * `down or height - 1`); a pair that writes neither is refused.
 *
 * vkx_region_warp_dev: rotate.distort of TextRegionFlattener.build_flattened_text_regions (:603-608) and of
 * FlattenedTextRegion.to_post_rotated_flattened_text_region (:148-153): per pair cv.warpAffine(src, m, dsize) of an image
 * (uint8 x 3) and a mask (uint8) with the pair's own forward matrix, pixel for pixel vkx_warp_affine_u8_dev's.
 * Of the warped plane the window of dst_h x dst_w at (up, left) is written: the trim to the rotated mask's external box
 * (:617-628) is a second call on the boxes of vkx_region_extent_dev.  extract != 0: an image source pixel counts as 0 where
 * the pair's source mask is 0 (Mask.extract_image, :589). */
typedef struct vkx_region_warp_pair {
    const uint8_t *src_image;           /* device uint8 [src_h][src_w][3] */
    const uint8_t *src_mask;            /* device uint8 [src_h][src_w] */
    int64_t src_image_step, src_mask_step;
    int32_t src_h, src_w;
    float m[6];                         /* the forward 2 x 3 matrix of RotateState, row-major */
    int32_t up, left, dst_h, dst_w;     /* the window of the warped plane that is written */
    int64_t dst_image_off, dst_mask_off;
} vkx_region_warp_pair;
int vkx_region_warp_dev(vkx_ctx *ctx, const vkx_region_warp_pair *pairs_host, int n_pairs, int extract, uint8_t *dst,
                        size_t dst_bytes);
/* vkx_region_extent_dev: Mask.to_external_box (element/mask.py:614-633) of n dense masks [h][w] packed in `masks` at
 * offsets_host[i] with shapes_host[i] = (h, w): extents[i] = (up, down, left, right) of the pixels > 0, or -1 four times
 * for a mask without one.  extents: DEVICE int32 [n][4]; the caller copies it back and synchronises once. */
int vkx_region_extent_dev(vkx_ctx *ctx, const uint8_t *masks, size_t masks_bytes, const int64_t *offsets_host,
                          const int32_t *shapes_host, int n_masks, int32_t *extents);
/* vkx_region_resize_dev: FlattenedTextRegion.to_resized_flattened_text_region (:114-122): per pair the image as
 * cv.resize(INTER_CUBIC) and the mask as cv.resize((mask > 0) * 255, INTER_CUBIC) > 0, pixel for pixel
 * vkx_resize_cubic_u8_dev's. */
typedef struct vkx_region_resize_pair {
    const uint8_t *src_image;           /* device uint8 [src_h][src_w][3] */
    const uint8_t *src_mask;            /* device uint8 [src_h][src_w] */
    int64_t src_image_step, src_mask_step;
    int32_t src_h, src_w, dst_h, dst_w;
    int64_t dst_image_off, dst_mask_off;
} vkx_region_resize_pair;
int vkx_region_resize_dev(vkx_ctx *ctx, const vkx_region_resize_pair *pairs_host, int n_pairs, uint8_t *dst, size_t dst_bytes);
/* vkx_region_stack_dev: build_background_image_for_stacking (:732-745) and the fills of stack_flattened_text_regions
 * (:805-840) into fresh planes: page_image uint8 [h][w][3] and page_mask uint8 [h][w], dense, every pixel of both written
 * once: where a region covers a pixel with mask > 0 the pixel of the LAST such region and mask 1, elsewhere channel
 * (y + x) % 3 at 255, the others 0, and mask 0.  Regions are dense planes [h][w][3] / [h][w] with their box origin; a box
 * outside the page and a region plane that overlaps a page plane are refused. */
typedef struct vkx_region_stack_item {
    const uint8_t *image, *mask;
    int32_t h, w, up, left;
} vkx_region_stack_item;
int vkx_region_stack_dev(vkx_ctx *ctx, const vkx_region_stack_item *items_host, int n_items, uint8_t *page_image,
                         uint8_t *page_mask, int h, int w);
/* vkx_region_extend_masks_dev: TextRegionFlattener.get_bounding_extended_text_region_masks (:477-558), the masks that
 * build_flattened_text_regions starts from, for all text regions of a page: three launches whatever n_regions, into fresh
 * planes.  text_mask: DEVICE uint8 [page_h][page_w] with its row step (the pitch contract of this header), the union T of the
 * rasters of all text-region polygons (vkx_paint_polys_fresh_dev, mask only); read as != 0.  Per region one HOST record: its box
 * BB (inclusive, inside the page) and three (offset, count) ranges of (x, y) pairs in the HOST int32 table pts_host, page
 * coordinates: the original polygon O, the (possibly dilated) polygon D and the bounding rectangular polygon R.  With o, d, r the
 * cv.fillPoly rasters of the three (the raster of vkx_fill_poly_mask_u8: LINE_8 outline plus even-odd spans), every pixel p
 * of BB gets
 *     out(p) = (d(p) and not (r(p) and T(p) and not o(p))) or (r(p) and not T(p))
 * as uint8 0 / 1 in the dense plane [BB.h][BB.w] at dst_off of the packed buffer `dst`; every byte of it is written once, `dst`
 * needs no memset.  The host tables travel through the page-locked ring: the call does not synchronise while no polygon has
 * more than 64 vertices; with a larger one it waits for the crossing-overflow flag, and more than 64 crossings of one polygon
 * on a scanline are VKX_ERR_UNSUPPORTED (as in vkx_paint_polys_dev).  Refused (VKX_ERR_INVALID, nothing launched): a NULL
 * pointer, n_regions outside 1 .. 4096, a BB outside the page or with a side outside 1 .. 32767, a polygon of fewer than 1
 * point or with a vertex outside BB (the reference asserts that a filling polygon's box lies inside the target's box,
 * element/box.py:227-228), a destination outside `dst`, destinations that overlap one another, text_mask overlapping `dst`, a
 * row step shorter than a row or negative. */
typedef struct vkx_region_masks_rec {
    int32_t up, down, left, right;      /* BB, inclusive */
    int32_t o_off, o_cnt;               /* the ranges of O, D, R in pts_host, in points */
    int32_t d_off, d_cnt;
    int32_t r_off, r_cnt;
    int64_t dst_off;
} vkx_region_masks_rec;
int vkx_region_extend_masks_dev(vkx_ctx *ctx, const vkx_region_masks_rec *regions_host, int n_regions, const int32_t *pts_host,
                                const uint8_t *text_mask, ptrdiff_t text_mask_step, int page_h, int page_w, uint8_t *dst,
                                size_t dst_bytes);

/* ---- Mask.to_disconnected_polygons (element/mask.py:657-733) ---------------------------------------------------------------
 * vkx_mask_contours_dev: cv.findContours(mask * 255, RETR_TREE, method) of n_masks masks, of which the contours with hierarchy
 * parent -1 are returned (keep_internal=False): the outer borders of the components that no hole encloses, in the order of their
 * raster-first pixels.  Pixels > 0 are foreground, 8-connected; background is 4-connected and surrounds the plane.  Each border
 * is OpenCV's icvFetchContour trace from that first pixel; method VKX_CHAIN_APPROX_NONE keeps every border pixel,
 * VKX_CHAIN_APPROX_SIMPLE the pixels where the direction changes.  Restated from the published algorithm, not pinned against
 * a cv2 binary.  A record addresses its mask by device pointer and row step (the pitch contract of this header): a mask may be
 * a rectangle inside a page plane.  Eight launches whatever the masks hold, no synchronisation; label planes, start bitmaps and
 * contour lengths (about 9.2 bytes a pixel of the batch) are context scratch, kept until the context is destroyed.
 * Outputs (DEVICE, dense):
 *   n_contours int32 [n_masks]; contour_len, contour_off int32 [cap_contours]: the contours of mask 0, then of mask 1, ...;
 *   contour_off is a contour's first point in `points` int32 [cap_points][2] (x, y);
 *   totals int64 [n_masks][2]: the contours and the points the mask needs, always complete;
 *   status int32 [n_masks]: 0, or VKX_CONTOURS_SHORT (the batch needs more than cap_contours contours or cap_points points:
 *   n_contours is 0 for every mask, and contour_len, contour_off and points are not written at all -- call again with the sums
 *   of totals) ored with VKX_CONTOURS_GAVE_UP (a trace of this mask reached its cap of 8 * h * w + 8 steps, which a plane that
 *   stays unchanged during the call never does: the mask's contours are not to be used).
 * Refused (VKX_ERR_INVALID, nothing launched): a NULL pointer, n_masks outside 1 .. 4096, a side outside 1 .. 32767, a mask of
 * more than 2^31 - 8 pixels or a batch of more than 2^32, a row step shorter than a row or negative, an unknown method, a
 * negative capacity, outputs that overlap one another or a mask. */
#define VKX_CHAIN_APPROX_NONE 1
#define VKX_CHAIN_APPROX_SIMPLE 2
#define VKX_CONTOURS_SHORT 1
#define VKX_CONTOURS_GAVE_UP 2
typedef struct vkx_contour_mask {
    const uint8_t *mask;                /* device uint8 [h][w] */
    int64_t step;
    int32_t h, w;
} vkx_contour_mask;
int vkx_mask_contours_dev(vkx_ctx *ctx, const vkx_contour_mask *masks_host, int n_masks, int method, int cap_contours,
                          int cap_points, int32_t *n_contours, int32_t *contour_len, int32_t *contour_off, int32_t *points,
                          int64_t *totals, int32_t *status);

/* ---- char binding: the mask-overlap counts of PageTextRegionStep (pipeline/text_detection/page_text_region.py) ---------------
 * vkx_poly_overlap_counts_dev: the integer areas behind calculate_boxed_masks_intersected_ratio (:189-227) for every
 * (candidate, anchor) pair that strtree_query_intersected_polygons (:899-925) visits, i.e. for the pairing of precise polygons
 * with disconnected text regions (:1115-1149) and the binding of a page's chars to its precise text regions (:1160-1216).
 * polys_host: one HOST record a polygon: its box (up, left, h, w: Polygon.bounding_box) and the range [pts_off, pts_off +
 * pts_cnt) of its SELF-RELATIVE points (Polygon.self_relative_polygon.to_np_array()) in the HOST int32 table pts_host of (x, y)
 * pairs.  pairs_host: HOST int32 [n_pairs][2] as (candidate, anchor), indices into polys_host.  The tables are dense.
 * counts: DEVICE int32 [n_polys + n_pairs]: counts[i] is the raster area of polygon i -- the number of pixels that
 * cv.fillPoly(zeros((h, w)), [points], 1) sets (the raster of vkx_fill_poly_mask_u8: LINE_8 outline plus even-odd spans; what
 * falls outside the h x w box is clipped), Polygon.mask.np_mask.sum() --, counts[n_polys + k] the intersected area of pair k:
 * the pixels that both rasters set inside the intersection of the two boxes, 0 where the boxes do not meet (:200-218).  The
 * device does no division: intersected_area / base_area is the caller's (two ints, float64).
 * Every polygon is rasterised once into a bit plane of its own in context scratch (one bit a pixel, rows padded to 32-bit
 * words; h * ((w + 31) / 32) * 4 bytes a polygon).  Three launches and one memset whatever n_polys and n_pairs; every count is
 * written by one lane with a plain store, no atomics: a rerun gives identical bytes.  The host tables travel through the
 * page-locked ring: the call does not synchronise while no polygon has more than 64 points; with a larger one it waits for the
 * crossing-overflow flag, and more than 64 crossings of one polygon on a scanline are VKX_ERR_UNSUPPORTED (as in
 * vkx_paint_polys_dev).  n_polys == 0 with n_pairs == 0 returns at once.
 * Refused (VKX_ERR_INVALID, nothing launched): a negative count; a NULL pointer; a pair index outside [0, n_polys); a polygon
 * of fewer than 1 point or with a point range that is negative or overflows; a box side outside 1 .. 32767; a box origin
 * beyond +-2^30; bit planes of more than VKX_POLY_OVERLAP_MAX_SCRATCH bytes in all (the caller splits its candidates into
 * several calls, the anchors rasterised in each). */
#define VKX_POLY_OVERLAP_MAX_SCRATCH (1ll << 30)
typedef struct vkx_poly_overlap_rec {
    int32_t up, left, h, w;             /* the polygon's box */
    int32_t pts_off, pts_cnt;           /* its self-relative points in pts_host, in points */
} vkx_poly_overlap_rec;
int vkx_poly_overlap_counts_dev(vkx_ctx *ctx, const vkx_poly_overlap_rec *polys_host, int n_polys, const int32_t *pts_host,
                                const int32_t *pairs_host, int n_pairs, int32_t *counts);
/* vkx_mask_overlap_counts_dev: the same areas for box-attached masks that are not polygons (:189-227 itself).  One HOST record
 * a pair: the two DEVICE uint8 planes with their boxes (up, left, h, w) and row steps (bytes from a row to the next, at least
 * one row, unused with a single row: the pitch contract of this header; a plane may be a rectangle inside a larger one).
 * counts: DEVICE int64 [n_recs][3]: the sum of the bytes of (anchor & candidate) over the intersection of the two boxes (0
 * where they do not meet), the number of nonzero bytes of the anchor, the number of nonzero bytes of the candidate.  One launch,
 * no synchronisation, no atomics; n_recs == 0 returns at once.  Refused (VKX_ERR_INVALID, nothing launched): n_recs outside
 * 0 .. 65536, a NULL pointer or plane, a box side outside 1 .. 32767, a box origin beyond +-2^30, a row step shorter than a row
 * or negative, counts overlapping a plane. */
typedef struct vkx_mask_overlap_rec {
    const uint8_t *anchor, *candidate;
    int64_t anchor_step, candidate_step;
    int32_t anchor_up, anchor_left, anchor_h, anchor_w;
    int32_t candidate_up, candidate_left, candidate_h, candidate_w;
} vkx_mask_overlap_rec;
int vkx_mask_overlap_counts_dev(vkx_ctx *ctx, const vkx_mask_overlap_rec *recs_host, int n_recs, int64_t *counts);

/* ---- the set-operation mask of a list of elements (element/mask.py:126-244) -----------------------------------------------
 * Mask.from_boxes / from_polygons / from_masks / from_score_maps and, through generate_fill_by_*_mask, the DISTINCT / INTERSECT
 * forms of the fill_by_* families (element/image.py:371-665, mask.py:283-410, score_map.py:315-520): count(y, x) is the number
 * of list entries active at the pixel (an entry listed twice counts twice; a polygon counts once where its outline and its spans
 * both land) and dst = 1 where the mode's predicate holds (UNION count > 0, DISTINCT count == 1, INTERSECT count > 1), else 0.
 * The result does not depend on the order in which the entries are rasterised.  At most four launches whatever n, none when
 * n == 0 (dst is zeroed), into a fresh plane: every byte of the h x w window of dst is written, no byte of its padding.
 * One HOST record an entry: its kind, its window [up, up + h) x [left, left + w) in plane coordinates, and
 *   VKX_SET_BOX        nothing more: the whole window is active;
 *   VKX_SET_POLYGON    the range [pts_off, pts_off + pts_cnt) of pts_host (int32 (x, y) pairs, plane coordinates): the
 *                      cv.fillPoly raster of vkx_fill_poly_mask_u8; the window is the polygon's bounding box;
 *   VKX_SET_MASK_U8    plane: DEVICE (host for vkx_set_mask) uint8 [h][w] over the window, active where > 0;
 *   VKX_SET_SCORE_F32  plane: float32 [h][w] over the window, active where > 0.0 (ScoreMap.to_mask()).
 * plane_step and dst_step are row steps in bytes (at least one row, unused with a single row: the pitch contract of this
 * header).  windows (optional, window_bytes bytes): entry e's own active raster, dense h_e x w_e at byte window_off_e; with
 * VKX_SET_WINDOWS_GATED ORed into mode it is ANDed with dst (the window a non-unique fill_by_masks / fill_by_score_maps fills
 * through).  The bytes between the first and the last polygon window are zeroed; windows of different entries may not share
 * bytes unless the entries are equal.  Refused (VKX_ERR_INVALID, nothing launched, dst untouched): n < 0 or above 65536, a NULL
 * dst, a plane side outside 1 .. 32767, an unknown kind or mode, a window outside h x w, a polygon vertex outside its window, a
 * point range outside pts_host, plane_step or dst_step shorter than the row or negative, a NULL plane for a mask or score map,
 * window_bytes too small, an element plane, dst and windows that overlap one another.  _dev: asynchronous on the ctx stream
 * while no polygon has more than 64 vertices (the tables are consumed before the call returns). */
#define VKX_SET_BOX 0
#define VKX_SET_POLYGON 1
#define VKX_SET_MASK_U8 2
#define VKX_SET_SCORE_F32 3
#define VKX_SET_UNION 0
#define VKX_SET_DISTINCT 1
#define VKX_SET_INTERSECT 2
#define VKX_SET_WINDOWS_GATED 0x100
typedef struct vkx_set_elem {
    int32_t kind, up, left, h, w, pts_off, pts_cnt, reserved;
    const void *plane;
    int64_t plane_step;
    int64_t window_off;
} vkx_set_elem;
int vkx_set_mask_dev(vkx_ctx *ctx, const vkx_set_elem *elems_host, int n, const int32_t *pts_host, int n_pts, int mode, int h,
                     int w, uint8_t *dst, ptrdiff_t dst_step, uint8_t *windows, size_t window_bytes);
int vkx_set_mask(vkx_ctx *ctx, const vkx_set_elem *elems_host, int n, const int32_t *pts_host, int n_pts, int mode, int h, int w,
                 uint8_t *dst, ptrdiff_t dst_step, uint8_t *windows, size_t window_bytes);

/* ---- fill_text_line_to_seal_impression (engine/seal_impression/text_line_slot_filler.py:28-205) --------------------------
 * vkx_seal_fill_dev builds the text-line score map of EVERY seal impression of a page: three launches whatever the number of
 * seals and chars, no synchronisation.  The records are HOST tables; the geometry in them (resized width, rotation matrix and
 * size, destination origin, the out-of-bound skip) is the caller's, every pixel is the call's:
 *   per char (:73-102) the glyph's score map (float32) resized with cv.resize(interpolation) and clipped to [0, 1]
 *   (ScoreMap.to_resized_score_map), or -- a glyph without one -- its image (uint8, 1 or 3 channels) as the mask any(image > 0),
 *   resized as (mask * 255) in uint8 arithmetic and thresholded > 0 (Mask.to_resized_mask); a source whose shape is already
 *   glyph_h x plane_w is copied as it is.  The result fills rows glyph_up .. of a zero plane of plane_h x plane_w (:78, :88);
 *   cv.warpAffine(plane, m, (rot_w, rot_h)) (:135-143; bilinear, constant 0 border, pixel for pixel vkx_warp_affine_f32_dev's;
 *   identity != 0: rotate.distort's nop for an angle of 0, the plane itself), filled at (dst_up, dst_left) of its seal's map
 *   keeping the maximum (:167-172: `mat < value` replaces, so neither a NaN nor a -0.0 ever does);
 *   per seal the internal text line's float32 score map, or its uint8 mask plane converted value for value, as a plain
 *   overwrite of its box after all chars (:181-192), then map * float32(alpha) / max(map) in float32 (:202-203): an all-zero
 *   map divides 0 by 0 and is NaN throughout, as in the reference.
 * Interpolations: the five codes a text line samples (VKX_INTER_NEAREST_EXACT, _LINEAR_EXACT, _CUBIC, _LANCZOS4, _AREA); AREA
 * shrinks only.  A source is a DEVICE plane with its row step in bytes
 * (the pitch contract of this header: at least one row, unused with a single row), or, with VKX_SEAL_SRC_HOST added to its
 * kind, a plane inside the HOST block `planes_host`, `src` being its byte offset there: the block travels with the tables as one
 * staged upload.  The chars of a seal are consecutive in the table (ascending `seal`).  dst: DEVICE float32, `dst_floats` long;
 * seal i is the dense plane [h][w] at dst_off floats; every element of it is written, dst needs no memset.
 * Refused (VKX_ERR_INVALID, nothing launched): a NULL pointer, n_chars outside 0 .. 4096, n_seals outside 1 .. 256, a side
 * outside 1 .. 32767, a row step shorter than its row or negative, glyph rows outside the char plane, a char destination box
 * or an internal box outside its seal, an unknown interpolation code or source kind, a VKX_INTER_AREA enlargement, a seal
 * destination outside dst, seal destinations that overlap one another, a device source that overlaps dst, a host source
 * outside planes_host. */
#define VKX_SEAL_SRC_F32 0
#define VKX_SEAL_SRC_U8C1 1
#define VKX_SEAL_SRC_U8C3 2
#define VKX_SEAL_SRC_HOST 16
#define VKX_SEAL_INTERNAL_NONE (-1)
typedef struct vkx_seal_char {
    const void *src;                    /* the glyph: float32 [src_h][src_w] or uint8 [src_h][src_w][1 or 3] */
    int64_t src_step;                   /* bytes */
    int32_t src_kind;                   /* VKX_SEAL_SRC_* */
    int32_t src_h, src_w;
    int32_t glyph_h;                    /* the glyph is resized to glyph_h x plane_w (equal to the source: copied) */
    int32_t interpolation;              /* VKX_INTER_* */
    int32_t plane_h, plane_w, glyph_up; /* the char plane (text line height x resized width), the row the glyph starts at */
    int32_t identity;
    float m[6];                         /* the forward 2 x 3 matrix of RotateState, row-major */
    int32_t rot_h, rot_w;               /* the rotated plane */
    int32_t seal, dst_up, dst_left;     /* its seal and origin there */
} vkx_seal_char;
typedef struct vkx_seal_rec {
    int32_t h, w;
    int64_t dst_off;                    /* floats */
    double alpha;
    const void *internal;               /* the internal text line: float32 score map or uint8 mask plane */
    int64_t internal_step;              /* bytes */
    int32_t internal_kind;              /* VKX_SEAL_INTERNAL_NONE, VKX_SEAL_SRC_F32 or VKX_SEAL_SRC_U8C1 (+ VKX_SEAL_SRC_HOST) */
    int32_t internal_up, internal_left, internal_h, internal_w;
} vkx_seal_rec;
int vkx_seal_fill_dev(vkx_ctx *ctx, const vkx_seal_char *chars_host, int n_chars, const vkx_seal_rec *seals_host, int n_seals,
                      const void *planes_host, size_t planes_host_bytes, float *dst, size_t dst_floats);

/* ---- render_text_line_meta, the pixel half (engine/font/freetype.py:314-380, :600-837) ----------------------------------------
 * vkx_text_lines_dev renders EVERY text line of a page from its glyph bitmaps: two launches whatever the number of lines and
 * chars, no synchronisation.  The records are HOST tables; every geometric decision in them (char boxes, resized shape, pad,
 * trim index, which chars the clean-up names) is the caller's and depends on no pixel, every pixel is the call's:
 *   the paste (:314-380): a plane of paste_h x paste_w, image 255, mask 0, score map 0.0; per char in table order, where its glyph
 *   (uint8 [glyph_h][glyph_w][channels]) is > 0 (any channel of a 3-channel LCD glyph) the image takes the line's colour
 *   (1 channel: cvtColor(RGBA2RGB) drops the alpha) or, LCD, ((1 - glyph / 255.0) * 255) truncated, in float64 as numpy has it
 *   (not 255 - glyph), or the glyph's own paste plane where the caller formed one (a gamma other than 1), and the mask 1; over the whole char box the score map keeps the maximum of the glyphs' score maps;
 *   the resize (:618-642; resized != paste shape): cv.resize(interpolation) of the image, of (mask * 255) then > 0
 *   (Mask.to_resized_mask) and of the score map then clipped to [0, 1] (ScoreMap.to_resized_score_map);
 *   the pad and the trim: the (resized) plane sits at (pad_up, pad_left) of a plane of 255 / 0 / 0.0, whose top left
 *   out_h x out_w pixels are the output;
 *   the clean-up of a trimmed char (:693-731, cleanup != 0; boxes {up, left, height, width} in the padded plane): inside
 *   trimmed_box, where the mask of glyph trimmed_char (resized to the box as a mask when the shapes differ) is set the image is
 *   255 and the mask 0, and the score map is 0; then inside kept_box the score map keeps the maximum with the score map of
 *   glyph kept_char (resized to the box and clipped when the shapes differ).
 * Interpolations: the five codes a text line samples (VKX_INTER_NEAREST_EXACT, _LINEAR_EXACT, _CUBIC, _LANCZOS4, _AREA); AREA
 * shrinks only.  `blob_host` is ONE host block holding the glyph bitmaps, score maps (float32, offsets multiples of 4) and paste
 * planes, dense, at the byte offsets of the char records (-1: none); it travels with the tables as one staged upload.  The chars
 * of a line are consecutive in the table (ascending `line`; trimmed_char / kept_char count from the line's first).  dst: DEVICE,
 * `dst_bytes` long, aligned to 4 bytes; per line the dense planes image uint8 [out_h][out_w][3] at image_off, mask uint8
 * [out_h][out_w] at mask_off and, has_score != 0 (exactly the 1-channel lines), score map float32 [out_h][out_w] at score_off
 * (a multiple of 4), all in bytes; every element of them is written, dst needs no memset.
 * Refused (VKX_ERR_INVALID, nothing launched): a NULL pointer, n_chars outside 1 .. 65536, n_lines outside 1 .. 4096, a line
 * without chars, a side outside 1 .. 32767, a negative pad, a colour outside 0 .. 255, a char box outside its line's pasted plane,
 * a kept box outside the output, a clean-up char outside its line, an unknown interpolation code, a VKX_INTER_AREA enlargement
 * (of a line or of a clean-up glyph), a blob offset out of range or misaligned, a destination outside dst or misaligned,
 * destinations that overlap one another. */
typedef struct vkx_text_char {
    int64_t image_off;                  /* blob: uint8 [glyph_h][glyph_w][channels of its line] */
    int64_t score_off;                  /* blob: float32 [glyph_h][glyph_w]; -1 for the glyphs of an LCD line */
    int64_t paste_off;                  /* blob: uint8 [glyph_h][glyph_w][3], what an LCD glyph pastes; -1: the gamma-1 value */
    int32_t glyph_h, glyph_w;
    int32_t line;
    int32_t up, left;                   /* the char box in the pasted plane: it has the glyph's shape */
    int32_t reserved;
} vkx_text_char;
typedef struct vkx_text_line {
    int32_t channels;                   /* of its glyphs: 1 (default, monochrome) or 3 (LCD) */
    int32_t color[3];                   /* the glyph colour of a 1-channel line */
    int32_t paste_h, paste_w;
    int32_t resized_h, resized_w;       /* equal to the pasted plane: not resized */
    int32_t interpolation;              /* VKX_INTER_* */
    int32_t pad_up, pad_left;
    int32_t out_h, out_w;
    int32_t has_score;
    int32_t cleanup, trimmed_char, kept_char;
    int32_t trimmed_box[4], kept_box[4];
    int32_t reserved;
    int64_t image_off, mask_off, score_off;   /* bytes */
} vkx_text_line;
int vkx_text_lines_dev(vkx_ctx *ctx, const vkx_text_char *chars_host, int n_chars, const vkx_text_line *lines_host, int n_lines,
                       const void *blob_host, size_t blob_bytes, uint8_t *dst, size_t dst_bytes);

/* ---- the page's symbol, barcode and frame layers (pipeline/text_detection/page_non_text_symbol.py:107-169 after
 * engine/image/selector.py:98-101; engine/barcode/qr.py:81-93 and code39.py:137-148; page_text_line_bounding_box.py:94-147) -------
 * vkx_page_layers_dev builds EVERY such layer of a page: at most two launches whatever the number of layers (one without symbol
 * records), no synchronisation.  The records are a HOST table; every draw and every box in them is the caller's, every pixel
 * is the call's, each operation rounded once in float32:
 *   VKX_LAYER_SYMBOL_RGBA  source uint8 [src_h][src_w][4]; r = cv.resize(source, (out_w, out_h), INTER_CUBIC) (equal shapes: the
 *     source itself); the image uint8 [out_h][out_w][3] = r[..., :3] at image_off; with a = r[..., 3] and m = max(a) over the
 *     record the plane float32 [out_h][out_w] = ((float32(a) / 255) * float32(alpha)) / (float32(m) / 255) at alpha_off; m == 0
 *     divides 0 by 0 and the plane is NaN throughout, as in the reference;
 *   VKX_LAYER_SYMBOL_GRAY  source uint8 [src_h][src_w]; g resized likewise; the plane is g > 0 ? float32(alpha) : 0, the image
 *     the constant `color`;
 *   VKX_LAYER_SCORE  source a uint8 module mask [src_h][src_w]; s = mask ? float32(alpha) : 0; where the shapes differ the plane
 *     is cv.resize(s, INTER_CUBIC) on float32 clipped to [0, 1] (ScoreMap.to_resized_score_map), else s; no image;
 *   VKX_LAYER_FRAME  no source; of a plane src_h x src_w that holds float32(alpha) on a ring of `thickness` pixels and 0 inside,
 *     the window of rows trim[0] .. src_h - 1 - trim[1] and columns trim[2] .. src_w - 1 - trim[3], which has out_h x out_w.
 * A source is dense: at byte offset src_off of the HOST block `blob_host`, which travels with the table as one staged upload, or
 * (src_off == -1) the DEVICE array src_dev.  dst: DEVICE, `dst_bytes` long, aligned to 4 bytes; the planes are dense, at the
 * byte offsets of the records (alpha_off a multiple of 4); every element of them is written, dst needs no memset.
 * Refused (VKX_ERR_INVALID, nothing launched): a NULL pointer, n_layers outside 1 .. 4096, an unknown kind, a side outside
 * 1 .. 32767, a colour outside 0 .. 255, an alpha that is NaN or outside [0, 1], a frame whose thickness is below 1 or leaves
 * an interior of fewer than two rows or columns (the reference's asserts), whose trims leave no window or whose output is not
 * that window, a blob offset out of range, a device source that overlaps dst, a destination outside dst, misaligned, or
 * overlapping another. */
#define VKX_LAYER_SYMBOL_RGBA 0
#define VKX_LAYER_SYMBOL_GRAY 1
#define VKX_LAYER_SCORE 2
#define VKX_LAYER_FRAME 3
typedef struct vkx_page_layer {
    int32_t kind;                       /* VKX_LAYER_* */
    int32_t src_h, src_w;               /* the source; VKX_LAYER_FRAME: the untrimmed plane */
    int32_t out_h, out_w;
    int32_t color[3];                   /* VKX_LAYER_SYMBOL_GRAY */
    int32_t thickness;                  /* VKX_LAYER_FRAME */
    int32_t trim[4];                    /* VKX_LAYER_FRAME: up, down, left, right */
    int32_t reserved;
    double alpha;
    int64_t src_off;                    /* blob, bytes; -1: src_dev */
    const void *src_dev;
    int64_t image_off, alpha_off;       /* dst, bytes; image_off is read for the symbol kinds only */
} vkx_page_layer;
int vkx_page_layers_dev(vkx_ctx *ctx, const vkx_page_layer *layers_host, int n_layers, const void *blob_host, size_t blob_bytes,
                        uint8_t *dst, size_t dst_bytes);

/* ---- text-line labels: quad interpolation and the box masks (element/score_map.py:139-283, :562-588;
 * pipeline/text_detection/page_text_line_label.py:156-306) ---------------------------------------------------------------------
 * One HOST record a quad, its vertices point0 .. point3 as ScoreMap.from_quad_interpolation holds them: x / y the rounded
 * integer vertices in plane coordinates (their extremes are the polygon's bounding box, and moved to its corner they are what
 * cv.fillPoly rasterises: vkx_fill_poly_mask_u8's raster), sx / sy the float32 NpVec.from_point values of the self-relative
 * vertices, and which of the two interpolated components the quad stores.
 * Per pixel (px, py) of the bounding box, the reference's arithmetic as numpy 2 evaluates it: q = (px, py) - vertex 0 in
 * float64; b1 = v1 - v0, b2 = v3 - v0, b3 = ((v0 - v1) - v3) + v2 and a = b2 x b3 in float32; b = float32(b3 x q - b1 x b2) and
 * c = float32(b1 x q) from float64 cross products; |a| < 0.001: v = -c / b, else the two roots (-b +- sqrt(b * b - (4a) * c)) *
 * float32(0.5 / a) in float32, every product, difference, root and quotient rounded once; of the two roots the one that lies in
 * [0, 1] on more pixels of the quad's raster is kept for the WHOLE quad, the positive one on a tie.  v is clipped to [0, 1];
 * u = float32((q.x - b2.x * v) / dx) in float64 where |dx| > |dy| and dx != 0 (dx = b1.x + b3.x * v, dy likewise), else the same
 * from y where dy != 0, else 0, clipped.  Outside the raster both are 0.
 * vkx_quad_interp_fill_dev: the stored component of every quad, in list order, onto dst (DEVICE float32, dense [h][w]) where
 * it is > 0 (a NaN never is): VKX_FILL_PLAIN overwrites, VKX_FILL_KEEP_MAX writes where dst < value, VKX_FILL_KEEP_MIN where
 * dst > value; with VKX_QUAD_FRESH_ONE ORed into mode dst is not read: it counts as 1.0f everywhere before the fills and every
 * element of it is written (a map born by ScoreMap.from_shape(value=1.0)).  zero_where (optional; DEVICE uint8, dense [h][w]): after the fills dst is 0.0f where it is 0.  At most two
 * launches whatever n_quads (the count of the roots, then the fill over the tiles of dst), no synchronisation.
 * vkx_quad_interp_uv_dev: (u, v) of ONE quad over its bounding box, DEVICE float32 dense [bh][bw][2], every element written.
 * Refused (VKX_ERR_INVALID, nothing launched): a NULL pointer, h or w outside 1 .. 32768, n_quads outside 0 .. 2^24 - 1, an
 * unknown component or mode, a quad whose bounding box leaves the plane (for the uv form: a side above 32768, or uv_floats
 * other than 2 * bh * bw), dst and zero_where that overlap. */
#define VKX_QUAD_U 0
#define VKX_QUAD_V 1
#define VKX_QUAD_FRESH_ONE 0x100
typedef struct vkx_quad {
    int32_t x[4], y[4];
    float sx[4], sy[4];
    int32_t component;                  /* VKX_QUAD_U or VKX_QUAD_V */
    int32_t reserved[3];
} vkx_quad;
int vkx_quad_interp_fill_dev(vkx_ctx *ctx, const vkx_quad *quads_host, int n_quads, int mode, int h, int w, float *dst,
                             const uint8_t *zero_where);
int vkx_quad_interp_uv_dev(vkx_ctx *ctx, const vkx_quad *quad_host, float *uv, size_t uv_floats);
/* The three masks of PageTextLineLabelStep in ONE launch whatever the number of boxes, no synchronisation.  boxes_host: HOST
 * int32 {up, left, height, width} records, the first n_text the text-line boxes, the next n_dilated the dilated-only boxes.
 * DEVICE uint8 dense [h][w], every byte written: text_mask = 1 under a text-line box; boundary_mask (optional) = 1 under a
 * dilated-only box and no text-line box; both_mask (optional) = 1 under either.  Refused: a NULL ctx, text_mask or (with
 * boxes) table, h or w outside 1 .. 32768, a count outside 0 .. 2^24 - 1, a box with a side below 1 or outside the plane,
 * masks that overlap. */
int vkx_box_label_masks_dev(vkx_ctx *ctx, const int32_t *boxes_host, int n_text, int n_dilated, int h, int w, uint8_t *text_mask,
                            uint8_t *boundary_mask, uint8_t *both_mask);

/* ---- batch collate (vkit_amd/torch_bridge.py) ----------------------------------------------------------------------------
 * The samples of a batch -- crops of several pages, each plane a dense block at its own device address -- into the dense batch
 * tensors a training loop consumes, in at most TWO launches whatever the batch size, no synchronisation.  The reference has no
 * such step (its samples leave as numpy arrays and the consumer stacks them); the arithmetic is fixed here so that it can be
 * checked bit for bit (tests/collate_restate.py).
 * Image launch (n_images > 0): images_host[i].src is a dense uint8 [height][width][3] block at ANY byte address (a view into a
 * packed buffer need not be dword aligned: an aligned source is read as dwords, another byte by byte).  norm->dst is the batch:
 * [n_images][3][height][width] (channels_first) or [n_images][height][width][3], dense, of norm->dtype, aligned to its
 * element.  VKX_COLLATE_U8 is the plain transpose / copy; the float types are
 *     out = (float32(x) - mean[c]) * scale[c]
 * with ONE float32 subtraction and ONE float32 multiplication (never fused), and for F16 / BF16 one more rounding to nearest
 * even.  (torch_bridge passes mean[c] = float32(255 mean_c), scale[c] = float32(1 / (255 std_c)), each worked out in float64
 * and rounded once.)  mean and scale are finite.
 * Plane launch (n_planes > 0): planes_host[i] copies `bytes` bytes from src to dst (label planes: uint8 masks and float32
 * score maps into their place in a batch tensor), 16 bytes a lane where src and dst are both 16-byte aligned, single bytes
 * otherwise.
 * The tables are HOST tables; every src and dst is a DEVICE pointer.  Refused (VKX_ERR_INVALID, nothing launched, nothing
 * written): a NULL ctx, a NULL table with a non-zero count, norm NULL with images, a NULL src or dst, a count below 0,
 * n_images above 65535, n_planes above 2^20, height or width outside 1 .. 32768, a plane of 0 bytes or of 2^31 and more, an unknown
 * dtype, channels_first other than 0 / 1, a dst not aligned to its element, a mean or scale that is not finite, two
 * destinations that overlap, a destination that overlaps a source. */
#define VKX_COLLATE_U8 0
#define VKX_COLLATE_F32 1
#define VKX_COLLATE_F16 2
#define VKX_COLLATE_BF16 3
typedef struct vkx_collate_image {
    const uint8_t *src;   /* device, uint8 [height][width][3], dense */
} vkx_collate_image;
typedef struct vkx_collate_plane {
    const void *src;      /* device */
    void *dst;            /* device */
    size_t bytes;
} vkx_collate_plane;
typedef struct vkx_collate_norm {
    void *dst;                /* device, the image batch */
    int32_t height, width;    /* of every source */
    int32_t dtype;            /* VKX_COLLATE_* */
    int32_t channels_first;   /* 1: [n][3][h][w]; 0: [n][h][w][3] */
    float mean[3], scale[3];
} vkx_collate_norm;
int vkx_collate_dev(vkx_ctx *ctx, const vkx_collate_image *images_host, int n_images, const vkx_collate_plane *planes_host,
                    int n_planes, const vkx_collate_norm *norm);

/* ---- JPEG encode (vkit_amd/element/image.py: Image.to_file, to_jpeg_bytes, encode_jpeg_images) ------------------------------
 * Image.to_file of the reference (image.py:351-359: to_rgb_image, to_pil_image, PIL's save) for a path Pillow writes as JPEG, for
 * a whole batch: every image becomes the file `PIL.Image.fromarray(mat).save(f, format='JPEG', quality=quality)` writes with
 * Pillow 12.2.0 / libjpeg-turbo 3.1.4.1 -- SOI, APP0 (JFIF 1.1, density 1 x 1, unit 0), one DQT per table, SOF0 (baseline; three
 * channels: sampling 2x2, 1x1, 1x1), one DHT per table (the Annex K tables), SOS, the scan without restart markers, EOI --
 * byte for byte (tests/jpeg_encode_restate.py, tests/golden/jpeg_encode.npz).
 * images_host is a HOST table of n records; every src is a DEVICE pointer to a DENSE uint8 [h][w][cn] block, cn 1 (one
 * component) or 3.  quality 0 .. 100 as in vkx_jpeg_roundtrip_u8 (0 scales the tables as 1).  bgr 1: channel 2 carries the red
 * weight (cv.imencode, vkx_jpeg_roundtrip_u8); bgr 0: channel 0 does (Pillow's mode RGB, Image in RGB mode).
 * out (device, `capacity` bytes) takes the files packed back to back: image i is out[offsets[i] .. offsets[i + 1]), offsets
 * (device, int64 [n + 1], 8-byte aligned) is written completely and offsets[n] is the total.  When the total exceeds capacity
 * nothing is written at or past out + capacity, offsets is complete all the same and the call returns VKX_OK: the caller reads
 * offsets[n] and calls again with a buffer of that size.
 * Eight launches and one memset whatever n is, no synchronisation; the scratch (140 bytes of coefficients, bit counts and offsets
 * plus 208 bytes of unstuffed stream per 8 x 8 block, dummy blocks included) belongs to the context.
 * Refused (VKX_ERR_INVALID, nothing launched, nothing written): a NULL argument or src, n outside 1 .. 65535, h or w outside
 * 1 .. 32768, cn other than 1 / 3, quality outside 0 .. 100, bgr other than 0 / 1, a negative capacity, offsets not aligned, out
 * or offsets overlapping a source or each other, more than 2^26 blocks in one call. */
typedef struct vkx_jpeg_image {
    const uint8_t *src;   /* device, uint8 [h][w][cn], dense */
    int32_t h, w, cn;
} vkx_jpeg_image;
int vkx_jpeg_encode_u8_dev(vkx_ctx *ctx, const vkx_jpeg_image *images_host, int n, int quality, int bgr, uint8_t *out,
                           long long capacity, int64_t *offsets);

/* ---- per-kernel timing -----------------------------------------------------------------
 * When enabled, every kernel launch is bracketed by a hipEvent pair recorded on the ctx
 * stream; vkx_ctx_collect_timings synchronises and folds them into per-kernel totals.
 * enabled = 2: only the large kernels (k_chain_fused, k_np_draw) are bracketed -- an event pair costs a few microseconds of
 * stream time, which a step of a dozen microsecond kernels notices. */
int vkx_ctx_set_timing(vkx_ctx *ctx, int enabled);
int vkx_ctx_collect_timings(vkx_ctx *ctx, int *n_kernels);
int vkx_ctx_get_timing(vkx_ctx *ctx, int index, const char **name, double *total_ms, long long *launches);
int vkx_ctx_reset_timings(vkx_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* VKX_H_ */
