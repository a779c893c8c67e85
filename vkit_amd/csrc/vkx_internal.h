// Internal definitions shared by the translation units of libvkx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <limits.h>
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vkx.h"

#define VKX_EXPORT extern "C" __attribute__((visibility("default")))

void vkx_set_error(const char *fmt, ...);

#define VKX_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            vkx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, \
                          __LINE__);                                                       \
            return VKX_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

// (the text of a refused requirement; vkd::ResizePlanner reports one in the name of its entry point)
#define VKX_REQUIRE_FORMAT "%s: requirement failed: %s"
#define VKX_REQUIRE(cond, msg)                                     \
    do {                                                           \
        if (!(cond)) {                                             \
            vkx_set_error(VKX_REQUIRE_FORMAT, __func__, msg);      \
            return VKX_ERR_INVALID;                                \
        }                                                          \
    } while (0)

// The pitch contract of vkx.h: a plane of `rows` rows of `row` units (bytes or elements, the unit of its stride) takes a
// stride of at least one row; with a single row the stride is never used.  A negative stride fails too.
#define VKX_REQUIRE_PITCH(stride, row, rows)                                                     \
    VKX_REQUIRE((rows) <= 1 || (ptrdiff_t)(stride) >= (ptrdiff_t)(row),                          \
                "row stride " #stride " shorter than a row, or negative")

// Do the byte ranges [p, p + (rows - 1) * pitch + row) of two planes overlap?  Pitches in bytes, already checked by
// VKX_REQUIRE_PITCH.
static inline bool vkx_planes_overlap(const void *a, int a_rows, ptrdiff_t a_pitch, size_t a_row, const void *b, int b_rows,
                                      ptrdiff_t b_pitch, size_t b_row)
{
    if (a_rows <= 0 || b_rows <= 0 || !a_row || !b_row) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (size_t)(a_rows - 1) * (size_t)a_pitch + a_row;
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (size_t)(b_rows - 1) * (size_t)b_pitch + b_row;
    return a0 < b1 && b0 < a1;
}
// The dense planes a call writes (and the ones it reads beside them): no two may share a byte.  NULL planes are skipped.
struct vkx_plane_bytes {
    const void *ptr;
    size_t bytes;
};
static inline bool vkx_planes_disjoint(const vkx_plane_bytes *planes, size_t n)
{
    for (size_t a = 0; a < n; a++)
        for (size_t b = a + 1; b < n; b++)
            if (planes[a].ptr && planes[b].ptr &&
                vkx_planes_overlap(planes[a].ptr, 1, 0, planes[a].bytes, planes[b].ptr, 1, 0, planes[b].bytes))
                return false;
    return true;
}
// Polygon.bounding_box of a char quad ((x, y) of 4 points): box = (up, left, height, width) of the points rounded half to even, still
// as doubles (exact): the site checks their range before it makes them ints.  False: a non-finite point.
static inline bool vkx_quad_box(const double q[8], double box[4])
{
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int k = 0; k < 4; k++) {
        if (!std::isfinite(q[2 * k]) || !std::isfinite(q[2 * k + 1])) return false;
        const double x = std::nearbyint(q[2 * k]), y = std::nearbyint(q[2 * k + 1]);
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
    }
    box[0] = y0; box[1] = x0; box[2] = y1 - y0 + 1; box[3] = x1 - x0 + 1;
    return true;
}
// The destinations [first, second) of a batched call, in the unit of its offsets: true when two of them overlap (sorts the list).
static inline bool vkx_ranges_overlap(std::vector<std::pair<long long, long long>> &ranges)
{
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++)
        if (ranges[i].first < ranges[i - 1].second) return true;
    return false;
}
// for the entry points that cannot run in place
#define VKX_REQUIRE_DISJOINT(...) \
    VKX_REQUIRE(!vkx_planes_overlap(__VA_ARGS__), "source and destination overlap (this operation cannot run in place)")

// The strides of every element of a multi-element remap ([sh, sw] -> [dh, dw]) and their source / destination overlap,
// all checked before the first launch.
static inline int vkx_check_elems(const vkx_elem *elems, int n_elems, int sh, int sw, int dh, int dw)
{
    for (int i = 0; i < n_elems; i++) {
        const vkx_elem &e = elems[i];
        const size_t esz = e.is_f32 ? 4 : 1, cn = e.cn > 0 ? (size_t)e.cn : 1;
        VKX_REQUIRE_PITCH(e.src_stride, (ptrdiff_t)(sw * cn), sh);
        VKX_REQUIRE_PITCH(e.dst_stride, (ptrdiff_t)(dw * cn), dh);
        VKX_REQUIRE_DISJOINT(e.src, sh, e.src_stride * (ptrdiff_t)esz, sw * cn * esz, e.dst, dh, e.dst_stride * (ptrdiff_t)esz,
                             dw * cn * esz);
    }
    return VKX_OK;
}

#define VKX_LAUNCH_CHECK()                                                 \
    do {                                                                     \
        hipError_t e__ = hipGetLastError();                                  \
        if (e__ != hipSuccess) {                                             \
            vkx_set_error("kernel launch failed in %s: %s", __func__, hipGetErrorString(e__)); \
            return VKX_ERR_HIP;                                              \
        }                                                                    \
    } while (0)

// A grow-only device scratch slot (owner maps, cell tables, staging for the host entry points).
struct vkx_scratch {
    void *ptr = nullptr;
    size_t cap = 0;
};

struct vkx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    vkx_scratch owner;    // int32 [dh, dw]
    vkx_scratch paint_owner;          // the ownership raster of vkx_paint_polys*_dev: all zero between calls (the resolve kernel clears what it reads)
    size_t paint_owner_zeroed = 0;    // ... bytes of it known to be zero
    vkx_scratch cells;    // CellRec [n_cells]
    vkx_scratch misc;     // small parameter blocks (layers, element descriptors)
    vkx_scratch tables;   // constant lookup tables (HSV division LUTs), uploaded once
    bool tables_ready = false;
    vkx_scratch stage[2]; // [0]: the planes of a host-pointer entry point (vkx_host_stage.h; the host forms of ellipse.hip, reduce.hip, poisson.hip,
                          // grid.hip, mls.hip and nprand.hip stage there themselves); [1]: a second block of the forms that stage themselves
                          // (the mask of ellipse.hip, the planes of vkx_paint_polys, the results of vkx_np_poisson_u8 and vkx_np_draw)
    vkx_scratch chain[3]; // ping-pong planes of the batched chain entry point; [2]: a tile buffer expanded to its int16 plane
    vkx_scratch chain_cells, chain_bins, chain_misc;   // cell records / tile bins / descriptors of the fused chain: its setup kernels
                                                       // run on the side stream while the shared slots above serve the compute stream
    hipEvent_t chain_setup_done = nullptr; // the side stream past the setup kernels of the current chain call
    hipEvent_t chain_done = nullptr;       // the pixel kernel of the last chain call (reads the three slots above)
    hipEvent_t lattices_ready = nullptr;   // vkx_chain_lattices_ready: the point of a stream the lattices are complete at
    bool lattices_armed = false;           // ... for the NEXT chain call only (a stale mark must not outlive the lattices it spoke of)
    vkx_scratch noise_table;          // int16 [65536] inverse-CDF table of vkx_noise_normal_i16 for noise_table_std
    double noise_table_std = 0.0;
    bool noise_table_fits8 = false;
    vkx_scratch np_tabs;              // jump constants + ziggurat tables of the numpy streams (nprand.hip), uploaded once
    vkx_scratch noise_rows;           // tiled noise of the fused chain: (row, tile column) -> slot offset records (fused.hip)
    vkx_scratch np_work[2];           // tile arrays of the numpy streams: the chunks of a call alternate (nprand.hip)
    vkx_scratch mls_work;                     // batched similarity_mls states (mls.hip): descriptors, handle tables, projected positions
    vkx_scratch camera_work;                  // camera states (camera.hip): descriptors, results, the depth values of the cubic curve
    vkx_scratch fog_work;                     // fog field (fog.hip): raw draws + the float64 centres of a level; a glass round's temporaries
    vkx_scratch jpeg_planes;                  // jpeg round trip (jpeg.hip): the decoded Y, Cb, Cr planes at their padded sizes
    vkx_scratch jpeg_encode_tables, jpeg_encode_work;   // jpeg encoder (jpeg_encode.hip): the staged records, Huffman codes and headers of the last call;
                                                        // its coefficients, bit and stuffing offsets and unstuffed streams
    vkx_scratch crop_windows, crop_planes;      // page cropping (crop.hip): the window and plane tables of the last call
    vkx_scratch combine_tables;               // combiner image engine (image_combine.hip): block bins + tile records of the last call
    vkx_scratch char_table, char_geo, char_layout, char_host;   // char masks (char_mask.hip): chars, setup results, tile layout,
                                                                // staging of the host form
    vkx_scratch char_owner;                   // ... the ownership planes: all zero between calls (the resolve clears what it reads)
    size_t char_owner_zeroed = 0;             // ... bytes of it known to be zero
    vkx_scratch heat_table, heat_geo, heat_host;   // char heatmap (char_heatmap.hip): template + quads + boxes + tile starts,
                                                   // setup results, staging of the host form
    vkx_scratch heat_planes;                  // ... the max / min / count planes (int [3][h * w])
    size_t heat_clean_page = 0;               // ... the page size they hold their initial values for (0: none)
    vkx_scratch rl_deviate, rl_planes;        // text-region labels (region_label.hip): the staged inputs of the two launches
    vkx_scratch rc_tables, rc_bitmap;         // text-region cropping (region_crop.hip): the staged tables; the preserved-char
                                              // bitmaps of the workgroups when they do not fit LDS
    vkx_scratch rf_tables;                    // text-region flattening (region_flatten.hip): the staged records and tap tables of the last call
    vkx_scratch rm_tables, rm_bits;           // text-region masks (region_masks.hip): the overflow flag + staged tables; the o / d / r bit planes of the last call
    vkx_scratch set_tables, set_planes;       // element set masks (element_sets.hip): the overflow flag + staged tables; the two index planes (int [2][h * w]) of the last call
    vkx_scratch seal_tables, seal_planes;     // seal impressions (seal_fill.hip): the staged records, tap tables and host planes of the last call; the char planes + per-seal maxima
    vkx_scratch text_tables, text_planes;     // text lines (text_line.hip): the staged records, resize tables and glyph blob of the last call; the pasted planes of its resized lines
    vkx_scratch layer_tables;                 // page layers (page_layers.hip): the staged records, resize tables, per-record maxima and host sources of the last call
    vkx_scratch quad_tables;                  // text-line labels (quad_interp.hip): the staged records, tile bins and vote counts of the last call
    vkx_scratch collate_tables;               // batch collate (collate.hip): the staged image and plane records of the last call
    vkx_scratch contour_tables, contour_planes;   // mask contours (contours.hip): the staged mask records; the label planes, start bitmaps, starts and
                                                  // contour lengths of the last call, sized to its batch and kept until the context is destroyed
    vkx_scratch ov_tables, ov_bits;           // char binding (polygon_overlap.hip): the overflow flag + staged tables (or the mask records); the polygons' bit planes of the last call
    vkx_scratch glass_win;                 // glass shuffle: the winner plane of a round's scatter (uint64 [h, w], zero between rounds)
    vkx_scratch pz_tabs, pz_work, pz_draws;   // rng.poisson on the device (poisson.hip): per-lam constants; block plan; raw draws + E rows
    bool pz_tabs_ready = false;

    // Host-array pipelines: two copy streams next to the compute stream (created on first use), a pool of events that
    // order them, and a page-locked ring through which the launch descriptors of the tile kernels reach the device
    // without a stream synchronisation (a launch returns while its descriptors are still in flight).
    hipStream_t copy_stream[2] = {nullptr, nullptr};   // [0] host -> device, [1] device -> host
    std::vector<hipEvent_t> order_events;              // reusable events of vkx_ctx_order / vkx_event_record
    unsigned char *desc_ring = nullptr;
    size_t desc_cap = 0, desc_off = 0;
    // Call-scoped hold: a block was handed out for a kernel to read in place (vkx_tables::mapped, HostStage::commit_mapped) and
    // that kernel is not queued yet, so no synchronisation protects the block.  While it is set a take that would wrap onto the
    // block or regrow the ring under it fails (VKX_ERR_NOMEM) and sets desc_hold to 2; the caller falls back to its copy path.
    int desc_hold = 0;

    // The table blocks of the last few resize geometries (resize.hip; PageResizingStep resizes seven elements with one
    // geometry: the tables are built and uploaded for the first one only).
    struct ResizeTabs {
        int key[6] = {-1, -1, -1, -1, -1, -1};    // taps (or 103 AREA, 105 LINEAR_EXACT), fixed point?, sh, sw, dh, dw
        vkx_scratch buf;                          // the block as its packer of vkx_resize_axes.h wrote it
        std::vector<int> meta;                    // host side: what the launch needs besides the block (row offsets, entry counts, ranges)
        unsigned long stamp = 0;
    };
    ResizeTabs resize_tabs[6];
    unsigned long resize_clock = 0;

    // Optional per-kernel timing with HIP events recorded on the launch stream (vkx_ctx_set_timing).
    int timing = 0;                           // 0 off, 1 every kernel, 2 only the large kernels (VKX_TIMED_MAJOR)
    struct TimedLaunch { int name_id; hipEvent_t start, stop; };
    std::vector<TimedLaunch> launches;       // recorded, not yet folded into the totals
    std::vector<hipEvent_t> event_pool;      // reusable events
    std::vector<std::string> timing_names;
    std::vector<double> timing_ms;
    std::vector<long long> timing_count;
};

// The current device is per-thread state: a ctx used from a thread other than its creator (or after the caller
// switched devices, e.g. torch.cuda.set_device) must see its own device while it launches on ctx->stream.
// Saves, sets and restores; free when the device is already current.
struct vkx_device_guard {
    int prev = -1;
    bool switched = false;
    explicit vkx_device_guard(const vkx_ctx *ctx);
    ~vkx_device_guard();
    vkx_device_guard(const vkx_device_guard &) = delete;
    vkx_device_guard &operator=(const vkx_device_guard &) = delete;
};

// RAII scope around ONE kernel launch: binds the ctx device for the launch and records a start / stop event pair on
// the ctx stream when timing is on.
struct vkx_timed {
    vkx_device_guard guard;
    vkx_ctx *ctx;
    int slot;
    vkx_timed(vkx_ctx *ctx, const char *kernel_name, bool major = false);
    ~vkx_timed();
};
#define VKX_TIMED(ctx, name) vkx_timed timed_scope__(ctx, name)
#define VKX_TIMED_MAJOR(ctx, name) vkx_timed timed_scope__(ctx, name, true)

int vkx_scratch_reserve(vkx_ctx *ctx, vkx_scratch *s, size_t bytes);
// `bytes` of page-locked host memory that stays untouched until everything queued on ctx->stream so far has run
// (ring allocation; wraps around with one stream synchronisation)
int vkx_desc_ring_take(vkx_ctx *ctx, size_t bytes, void **hptr);
// Small records between page-locked host memory and the device ON the compute stream, by a one-workgroup kernel that
// reads / writes the host memory through its device mapping: a hipMemcpyAsync of a few hundred bytes queues on the copy
// engines behind the multi-megabyte plane transfers of the other lanes of a host pipeline and stalls the kernels after
// it for the length of those transfers.  `bytes` a multiple of 4.  to_host falls back to hipMemcpyAsync when `host` is
// not mapped page-locked memory.
int vkx_small_to_device(vkx_ctx *ctx, void *dev, const void *ring_host, size_t bytes);
int vkx_small_to_host(vkx_ctx *ctx, void *host, const void *dev, size_t bytes);
hipStream_t vkx_stream_by_id(vkx_ctx *ctx, int id, int *rc);
const void *vkx_ring_device_ptr(const void *ring_host);              // a ring block as kernels address it (mapped host memory), or nullptr

static inline size_t vkx_align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The environment switches of INTEGRATION.md as the library reads them (a site keeps the value in a `static const`: once per process).
// vkx_env_int: the integer the variable holds, `unset` without it.  vkx_env_on: 0 for a value that begins with '0', 1 for any other,
// `unset` without the variable (-1 where a site tells "forced off" from "not set").
static inline int vkx_env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
static inline int vkx_env_on(const char *name, int unset) { const char *e = getenv(name); return e ? (e[0] == '0' ? 0 : 1) : unset; }

// The small tables a call builds on the host (edge lists, tile bins, descriptors, LUTs) on their way to the device: lay the
// parts out with add() (each starts on a 256-byte boundary), take() ONE ring block for all of them, write each part where
// at<T>(offset) points -- straight into the ring --, then deliver the block in the way the site has measured to be best:
// copy_to() (one hipMemcpyAsync on ctx->stream), small_to() (vkx_small_to_device) or mapped() (read, or written, in place).
struct vkx_tables {
    vkx_ctx *ctx;
    size_t bytes = 0;                  // the end of the last part: what take() asks for and the copies move
    unsigned char *host = nullptr;     // the ring block, after take()
    bool holds = false;                // mapped() set the ring's hold
    explicit vkx_tables(vkx_ctx *c) : ctx(c) {}
    ~vkx_tables() { release(); }
    vkx_tables(const vkx_tables &) = delete;
    vkx_tables &operator=(const vkx_tables &) = delete;

    size_t add(size_t n) { const size_t off = vkx_align256(bytes); bytes = off + n; return off; }
    int take(size_t n = 0) { if (n) add(n); return vkx_desc_ring_take(ctx, bytes, (void **)&host); }   // (n: a last, or the only, part)
    template <class T> T *at(size_t off) const { return (T *)(host + off); }
    int copy_to(void *dev) const           // ... to a base the caller reserved (at least `bytes`)
    {
        vkx_device_guard guard(ctx);
        VKX_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return VKX_OK;
    }
    int copy_to(vkx_scratch *s, size_t min_cap = 0)   // ... to s->ptr, reserved here with the site's minimum capacity
    {
        const int rc = vkx_scratch_reserve(ctx, s, bytes > min_cap ? bytes : min_cap);
        return rc ? rc : copy_to(s->ptr);
    }
    int small_to(void *dev) const { vkx_device_guard guard(ctx); return vkx_small_to_device(ctx, dev, host, bytes); }
    // The block as kernels address it, or nullptr where the ring cannot be mapped (the site falls back to a copy, or fails).  The
    // kernel that will read it is not queued yet, so the ring is held (vkx_ctx::desc_hold) until release() or the end of this object.
    unsigned char *mapped()
    {
        unsigned char *dev = (unsigned char *)const_cast<void *>(vkx_ring_device_ptr(host));
        if (dev && !ctx->desc_hold) { ctx->desc_hold = 1; holds = true; }
        return dev;
    }
    bool release()                     // true: a take was refused during the hold
    {
        const bool refused = holds && ctx->desc_hold == 2;
        if (holds) ctx->desc_hold = 0;
        holds = false;
        return refused;
    }
};
int vkx_stream_order(vkx_ctx *ctx, hipStream_t later, hipStream_t earlier);
void vkx_ctx_join_streams(vkx_ctx *ctx, hipStream_t main_stream);   // error exits of multi-stream calls: main after the side streams, ctx->stream = main
int vkx_chain_consume_lattices_mark(vkx_ctx *ctx);                   // staged chain paths: the compute stream waits for a pending lattices-ready mark
// out[i] = next_double of the PCG64 stream (state, inc) at its (i + 1)-th step (poisson.hip); asynchronous on the ctx stream
int vkx_pcg64_doubles_dev(vkx_ctx *ctx, const uint64_t *state, const uint64_t *inc, long long M, double *out);

// Plane copies between host and device staging: hipMemcpy2DAsync is an order of magnitude slower than a linear copy on
// this stack (12 ms instead of 1 ms for a 2048^2 RGB plane), so planes whose rows follow each other without gaps -- every
// numpy array the binding passes -- travel as ONE linear copy; only genuinely pitched planes take the 2D call.
static inline hipError_t vkx_copy_plane(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t row_bytes,
                                        size_t rows, hipMemcpyKind kind, hipStream_t stream)
{
    if (rows == 0 || row_bytes == 0) return hipSuccess;
    if (rows == 1 || (dst_pitch == row_bytes && src_pitch == row_bytes))
        return hipMemcpyAsync(dst, src, row_bytes * rows, kind, stream);
    return hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, row_bytes, rows, kind, stream);
}

static inline unsigned vkx_blocks(size_t n, unsigned per_block)
{
    size_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b);
}

// ---------------------------------------------------------------------------------------------
// Device helpers.  Everything here must agree bit-for-bit with oracle/vkx_oracle.c; the library
// is compiled with -ffp-contract=off so a*b+c is never fused unless written as fma().
// ---------------------------------------------------------------------------------------------
namespace vkd {

// OpenCV cvRound on x86: round-half-even, "integer indefinite" outside int32 / NaN.
__device__ __forceinline__ int cv_round(float v)
{
    if (!(fabsf(v) < 2147483648.f)) return INT_MIN;   // -2^31 itself converts to INT_MIN either way
    return __float2int_rn(v);
}
__device__ __forceinline__ int cv_round(double v)
{
    if (!(v >= -2147483648.5 && v < 2147483647.5)) return INT_MIN;
    return __double2int_rn(v);
}
// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba): the border rule of the uint8 Gaussian blur, shared by every kernel that reads
// a blur window (photo.hip, fused.hip, image_combine.hip).
__device__ __forceinline__ int reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * (len - 1) - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}
// The last of n >= 1 entries whose prefix is <= t: prefix(i) ascending, prefix(0) <= t.  (Which edge, quad or glyph owns item t of
// a launch laid out by a prefix sum; box_tile_pixel below is its use for the tiles of boxes; fused.hip and nprand.hip keep their
// own copies.)
template <class Prefix>
__device__ __forceinline__ int last_at_most(int n, int t, Prefix prefix)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix(mid) <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// The pixel of a lane where workgroup blockIdx.x is one TW x TH tile of an h x w plane, tiles_x tiles a row (the bins of
// vkx_tile_bins.h; a workgroup of fewer than TW * TH lanes has the first rows of its tile).  False: outside the plane.
template <int TW, int TH>
__device__ __forceinline__ bool tile_pixel(int tiles_x, int h, int w, int &x, int &y)
{
    const int t = blockIdx.x, ty = t / tiles_x, tx = t - ty * tiles_x;
    y = ty * TH + (int)threadIdx.x / TW;
    x = tx * TW + (int)threadIdx.x % TW;
    return y < h && x < w;
}
// ... where workgroup blockIdx.x is one TW x TH tile of one of n boxes: box g owns the tiles from first_tile(g) up to first_tile(g + 1)
// (a prefix the caller holds in its records) and width_of(g) is its width.  Returns the box, and the pixel (rx, ry) inside it -- the
// caller tests it against the sides.
template <int TW, int TH, class FirstTile, class WidthOf>
__device__ __forceinline__ int box_tile_pixel(int n, FirstTile first_tile, WidthOf width_of, int &rx, int &ry)
{
    const int t = blockIdx.x;
    const int g = last_at_most(n, t, first_tile);
    const int tiles_x = (width_of(g) + TW - 1) / TW, lt = t - first_tile(g);
    ry = (lt / tiles_x) * TH + (int)threadIdx.x / TW;
    rx = (lt % tiles_x) * TW + (int)threadIdx.x % TW;
    return g;
}
// ... the prefix an array (vkb::box_tile_starts)
template <int TW, int TH, class WidthOf>
__device__ __forceinline__ int box_tile_pixel(int n, const int *__restrict__ tile_start, WidthOf width_of, int &rx, int &ry)
{
    return box_tile_pixel<TW, TH>(n, [&](int i) { return tile_start[i]; }, width_of, rx, ry);
}
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One destination pixel of cv::remapBilinear on uint8, BORDER_CONSTANT 0.  X, Y are the source
// coordinate in 1/32 px.  The int16 weight table of OpenCV is (32-fy)(32-fx)*32 etc. (with the
// {32767,0,0,1} quirk at fy=fx=0); (sum*32 + 2^14) >> 15 == (sum + 512) >> 10 for every entry,
// the quirk entry included, so the table never needs to be materialised.
// PTR: `const uint8_t *` or the same in an explicit address space (a kernel that holds its planes as global-address-space
// pointers keeps FLAT instructions out of its code that way).
template <int CN, class Tap>
__device__ __forceinline__ void sample_taps_u8(Tap tap, int sh, int sw, int X, int Y, uint8_t *out)
{
    // tap(y, x, k): channel k of source pixel (y, x), asked for pixels inside the source only
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
    const int fx = X & 31, fy = Y & 31;
    if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
#pragma unroll
        for (int k = 0; k < CN; k++) out[k] = 0;
        return;
    }
    const bool x0 = sx >= 0, x1 = sx + 1 < sw, y0 = sy >= 0, y1 = sy + 1 < sh;
    const int w00 = (32 - fy) * (32 - fx), w01 = (32 - fy) * fx, w10 = fy * (32 - fx), w11 = fy * fx;
#pragma unroll
    for (int k = 0; k < CN; k++) {
        const int v0 = (x0 && y0) ? tap(sy, sx, k) : 0;
        const int v1 = (x1 && y0) ? tap(sy, sx + 1, k) : 0;
        const int v2 = (x0 && y1) ? tap(sy + 1, sx, k) : 0;
        const int v3 = (x1 && y1) ? tap(sy + 1, sx + 1, k) : 0;
        out[k] = (uint8_t)((v0 * w00 + v1 * w01 + v2 * w10 + v3 * w11 + 512) >> 10);
    }
}
// ... on a plane in memory.  The batched region warp (region_flatten.hip) reads its taps through a mask instead.
template <int CN, typename PTR = const uint8_t *>
__device__ __forceinline__ void sample_u8(PTR src, int sh, int sw, ptrdiff_t sstride, int X, int Y, uint8_t *out)
{
    sample_taps_u8<CN>([&](int y, int x, int k) { return (int)src[(ptrdiff_t)y * sstride + (ptrdiff_t)x * CN + k]; }, sh, sw, X, Y, out);
}

template <typename PTR = const float *>
__device__ __forceinline__ float sample_f32(PTR src, int sh, int sw, ptrdiff_t sstride_el, int X, int Y)
{
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
    const int fx = X & 31, fy = Y & 31;
    if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) return 0.f;
    const bool x0 = sx >= 0, x1 = sx + 1 < sw, y0 = sy >= 0, y1 = sy + 1 < sh;
    const PTR r0 = src + (ptrdiff_t)sy * sstride_el + sx;
    const PTR r1 = r0 + sstride_el;
    const float ax = fx * (1.f / 32), ay = fy * (1.f / 32);
    const float bx = 1.f - ax, by = 1.f - ay;
    const float w0 = by * bx, w1 = by * ax, w2 = ay * bx, w3 = ay * ax; // exact products (5 bit x 5 bit)
    const float v0 = (x0 && y0) ? r0[0] : 0.f;
    const float v1 = (x1 && y0) ? r0[1] : 0.f;
    const float v2 = (x0 && y1) ? r1[0] : 0.f;
    const float v3 = (x1 && y1) ? r1[1] : 0.f;
    const float p0 = v0 * w0, p1 = v1 * w1, p2 = v2 * w2, p3 = v3 * w3;
    return ((p0 + p1) + p2) + p3;
}

// cv.warpPerspective's source coordinate of destination pixel (x, y) in 1/32 px (imgwarp.cpp WarpPerspectiveInvoker): the
// inverse matrix evaluated in double per pixel, with the x terms of a row restarted at the start of every bw0-wide block.
// Shared by the warp kernels of remap.hip and the char-mask raster of char_mask.hip.
struct CoordPerspective { // warpPerspective: inverse matrix, per pixel in double, 32x32 blocks
    static constexpr bool kTile2D = true;
    double m[9];
    int bw0;
    struct Column {};
    struct Rows {};
    __device__ __forceinline__ Column column(int) const { return Column(); }
    __device__ __forceinline__ Rows rows(int, int) const { return Rows(); }
    __device__ __forceinline__ void at(const Column &, const Rows &, int, int x, int y, int &X, int &Y) const { (*this)(x, y, X, Y); }
    __device__ __forceinline__ void operator()(int x, int y, int &X, int &Y) const
    {
        const int xb = (x / bw0) * bw0, x1 = x - xb;
        const double X0 = m[0] * xb + m[1] * y + m[2];
        const double Y0 = m[3] * xb + m[4] * y + m[5];
        const double W0 = m[6] * xb + m[7] * y + m[8];
        double W = W0 + m[6] * x1;
        W = W ? 32 / W : 0;
        const double fX = fmax((double)INT_MIN, fmin((double)INT_MAX, (X0 + m[0] * x1) * W));
        const double fY = fmax((double)INT_MIN, fmin((double)INT_MAX, (Y0 + m[3] * x1) * W));
        X = vkd::cv_round(fX);
        Y = vkd::cv_round(fY);
    }
};

// The CoordPerspective of cv.warpPerspective(src, S, (dw, dh)) (no WARP_INVERSE_MAP: S inverted here, a singular S gives
// the zero matrix as cv::invert does).
__host__ __device__ inline CoordPerspective make_perspective(const double S[9], int dh, int dw)
{
    CoordPerspective c;
    auto at = [&](int r, int col) { return S[r * 3 + col]; };
    double d = at(0, 0) * (at(1, 1) * at(2, 2) - at(1, 2) * at(2, 1)) -
               at(0, 1) * (at(1, 0) * at(2, 2) - at(1, 2) * at(2, 0)) +
               at(0, 2) * (at(1, 0) * at(2, 1) - at(1, 1) * at(2, 0));
    if (d == 0.) {
        for (int i = 0; i < 9; i++) c.m[i] = 0;
    } else {
        d = 1. / d;
        c.m[0] = (at(1, 1) * at(2, 2) - at(1, 2) * at(2, 1)) * d;
        c.m[1] = (at(0, 2) * at(2, 1) - at(0, 1) * at(2, 2)) * d;
        c.m[2] = (at(0, 1) * at(1, 2) - at(0, 2) * at(1, 1)) * d;
        c.m[3] = (at(1, 2) * at(2, 0) - at(1, 0) * at(2, 2)) * d;
        c.m[4] = (at(0, 0) * at(2, 2) - at(0, 2) * at(2, 0)) * d;
        c.m[5] = (at(0, 2) * at(1, 0) - at(0, 0) * at(1, 2)) * d;
        c.m[6] = (at(1, 0) * at(2, 1) - at(1, 1) * at(2, 0)) * d;
        c.m[7] = (at(0, 1) * at(2, 0) - at(0, 0) * at(2, 1)) * d;
        c.m[8] = (at(0, 0) * at(1, 1) - at(0, 1) * at(1, 0)) * d;
    }
    const int BLOCK_SZ = 32;
    const int bh0 = BLOCK_SZ / 2 < dh ? BLOCK_SZ / 2 : (dh > 0 ? dh : 1);
    c.bw0 = BLOCK_SZ * BLOCK_SZ / bh0 < dw ? BLOCK_SZ * BLOCK_SZ / bh0 : (dw > 0 ? dw : 1);
    return c;
}

} // namespace vkd

// cross-translation-unit helpers
int vkx_hsv_tables(vkx_ctx *ctx, const void **out);                      // photo.hip
int vkx_gaussian_kernel_q8_host(int n, double sigma, uint16_t *kq);      // photo.hip
int vkx_chain_fused_try(vkx_ctx *ctx, const vkx_chain_item *items, int n_items);  // fused.hip
// the steps of the fused chain, for callers that queue them on streams of their choice (chain.hip); fused.hip
struct vkx_chain_plan;
int vkx_chain_plan_build(vkx_ctx *ctx, const vkx_chain_item *items, int n_items, vkx_chain_plan **out);   // VKX_ERR_UNSUPPORTED: not for the fused path
void vkx_chain_plan_free(vkx_chain_plan *p);
int vkx_chain_plan_setup_aside(vkx_ctx *ctx, vkx_chain_plan *p, hipEvent_t *done);      // side stream; *done (may be NULL: ran on ctx->stream): what the pixel kernels wait for
int vkx_chain_plan_noise_rows(vkx_ctx *ctx, vkx_chain_plan *p, int first, int count);   // on ctx->stream
int vkx_chain_plan_tiles(vkx_ctx *ctx, vkx_chain_plan *p, int first, int count);        // on ctx->stream
int vkx_chain_mark_done(vkx_ctx *ctx, hipStream_t stream);
// one chunk of VKX_NP_NORMAL_TILES jobs (nprand.hip): begin = tile states + draw pass, finish = carries, walks, tables; each on
// ctx->stream as it is when called.  `slot`: which of the two tile-array scratch slots the chunk uses.
struct vkx_np_chunk;
int vkx_np_jobs_check(const vkx_np_job *jobs, int n_jobs, const vkx_np_result *results_host);
int vkx_np_chunk_begin(vkx_ctx *ctx, const vkx_np_job *jobs, int n_jobs, vkx_np_result *results_host, int slot, vkx_np_chunk **out);
int vkx_np_chunk_finish(vkx_ctx *ctx, vkx_np_chunk *c);
void vkx_np_chunk_free(vkx_np_chunk *c);
int vkx_tile_remap_try(vkx_ctx *ctx, const vkx_elem *elems, int n_elems, int sh, int sw, const int32_t *src_vertices,
                       const int32_t *dst_vertices, int rows, int cols, int dh, int dw);  // fused.hip
// the tile buffer of a VKX_NP_NORMAL_TILES job of n samples (nprand.hip; read by the fused chain kernel)
struct vkx_np_tiles_shape {
    long long n_tiles;
    int slot_elems;
    size_t table_offset, slots_offset, bytes;
    double samples_per_tile;     // expectation: the first guess of "which tile holds sample i"
};
vkx_np_tiles_shape vkx_np_tiles_shape_of(long long n);
