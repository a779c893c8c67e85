// The batch collate of vkit_amd/torch_bridge.py on gfx950: the samples of a batch -- dense planes at arbitrary device addresses,
// crops of several pages -- into the dense batch tensors of the consumer, in at most two launches (include/vkx.h, "batch collate").
//
//   k_collate_images   the uint8 [h][w][3] sources into [n][3][h][w] or [n][h][w][3] of uint8 / float32 / float16 / bfloat16,
//                      out = (float32(x) - mean[c]) * scale[c].  Source and batch are both dense, so a sample is ONE run of
//                      h * w pixels and the rows never show: a lane takes groups of 4 pixels -- 12 source bytes, typed as bytes
//                      because a view into a packed buffer starts at any address; gfx950 reads global memory at any alignment
//                      and the compiler makes them ONE 12-byte load either way --, de-interleaves them in registers and writes one
//                      4-element store per plane (16 bytes of float32, 8 of the 16-bit types), or three for the interleaved layout.  The
//                      h * w % 4 pixels left over are written element by element by the first lanes of the sample's first
//                      workgroup.  grid (groups / 512, n): two groups a lane, both loaded before the first store.  No LDS.
//   k_collate_planes   the label planes: a table of (src, dst, bytes) copies of any sizes, each owning the run of workgroups its
//                      bytes take (8 KB a workgroup; the run is found by bisection of the records' first workgroups); 16 bytes a
//                      lane where both ends are 16-byte aligned, then the last bytes singly; bytes throughout otherwise.
// Both are bound by memory (3 B/px in and 3 / 6 / 12 B/px out; a plane byte in and out): no byte is read or written twice.
// The stores are typed with the alignment the destination is known to have (its element's), the compiler picks the widest
// instruction that alignment allows.
#include "vkx_internal.h"

#include <cstring>
#include <vector>

namespace {

constexpr int kBlock = 256;
constexpr int kGroupsPerLane = 2;                                  // 4-pixel groups of a lane
constexpr unsigned kGroupsPerBlock = kBlock * kGroupsPerLane;
constexpr unsigned kPlaneBlockBytes = kBlock * 16 * 2;             // of a plane, a workgroup
constexpr int kMaxImages = 65535, kMaxPlanes = 1 << 20, kMaxSide = 32768;

struct ImageParams {
    void *dst;
    unsigned pixels;          // h * w of a sample
    float mean[3], scale[3];
};
struct PlaneRec {             // what k_collate_planes reads: the ABI's record with its first workgroup
    const uint8_t *src;
    uint8_t *dst;
    unsigned bytes, first_block;
};

// round to nearest even; the values are finite (finite mean and scale), an overflow rounds to infinity as it should
__device__ __forceinline__ uint16_t bf16_bits(float v)
{
    const unsigned u = __float_as_uint(v);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <int kDtype> struct OutType;
template <> struct OutType<VKX_COLLATE_U8> {
    typedef uint8_t T;
    static __device__ __forceinline__ T of(unsigned x, float, float) { return (uint8_t)x; }
};
template <> struct OutType<VKX_COLLATE_F32> {
    typedef float T;
    static __device__ __forceinline__ T of(unsigned x, float m, float s) { return ((float)x - m) * s; }
};
template <> struct OutType<VKX_COLLATE_F16> {
    typedef _Float16 T;
    static __device__ __forceinline__ T of(unsigned x, float m, float s) { return (_Float16)(((float)x - m) * s); }
};
template <> struct OutType<VKX_COLLATE_BF16> {
    typedef uint16_t T;
    static __device__ __forceinline__ T of(unsigned x, float m, float s) { return bf16_bits(((float)x - m) * s); }
};

// four elements stored as one, at the alignment of an element
template <class T> struct __attribute__((packed, aligned(sizeof(T)))) Quad {
    T v[4];
};
typedef uint32_t __attribute__((aligned(1))) word_at_any_address;
typedef uint32_t words4 __attribute__((ext_vector_type(4)));
// (pointers that come out of a table are generic to the compiler: said to be global, they keep FLAT instructions out of the code)
#define VKX_GLOBAL(T) __attribute__((address_space(1))) T

template <int kDtype, bool kPlanar>
__global__ void __launch_bounds__(kBlock) k_collate_images(const vkx_collate_image *__restrict__ images, ImageParams p)
{
    typedef OutType<kDtype> O;
    typedef typename O::T T;
    const VKX_GLOBAL(uint8_t) *__restrict__ src = (const VKX_GLOBAL(uint8_t) *)images[blockIdx.y].src;
    T *__restrict__ dst = (T *)p.dst + (size_t)blockIdx.y * 3 * p.pixels;
    const unsigned groups = p.pixels >> 2;

    unsigned g[kGroupsPerLane];
    uint32_t in[kGroupsPerLane][3];
#pragma unroll
    for (int k = 0; k < kGroupsPerLane; k++) {
        g[k] = (blockIdx.x * kGroupsPerLane + k) * kBlock + threadIdx.x;
        if (g[k] >= groups) continue;
        const VKX_GLOBAL(word_at_any_address) *w = (const VKX_GLOBAL(word_at_any_address) *)(src + (size_t)g[k] * 12);
#pragma unroll
        for (int j = 0; j < 3; j++) in[k][j] = w[j];
    }
#pragma unroll
    for (int k = 0; k < kGroupsPerLane; k++) {
        if (g[k] >= groups) continue;
        auto byte = [&](int i) { return (in[k][i >> 2] >> (8 * (i & 3))) & 0xffu; };     // i: 3 * pixel + channel
        if (kPlanar) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Quad<T> q;
#pragma unroll
                for (int px = 0; px < 4; px++) q.v[px] = O::of(byte(3 * px + c), p.mean[c], p.scale[c]);
                *(Quad<T> *)(dst + (size_t)c * p.pixels + (size_t)g[k] * 4) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Quad<T> q;
#pragma unroll
                for (int e = 0; e < 4; e++) q.v[e] = O::of(byte(4 * j + e), p.mean[(4 * j + e) % 3], p.scale[(4 * j + e) % 3]);
                *(Quad<T> *)(dst + (size_t)g[k] * 12 + 4 * j) = q;
            }
        }
    }
    // the pixels past the last whole group, an element a lane
    const unsigned tail = 3 * (p.pixels & 3);
    if (blockIdx.x == 0 && threadIdx.x < tail) {
        const unsigned px = groups * 4 + threadIdx.x / 3, c = threadIdx.x % 3;
        const T v = O::of(src[(size_t)px * 3 + c], p.mean[c], p.scale[c]);
        dst[kPlanar ? (size_t)c * p.pixels + px : (size_t)px * 3 + c] = v;
    }
}

__global__ void __launch_bounds__(kBlock) k_collate_planes(const PlaneRec *__restrict__ recs, int n)
{
    const int r = vkd::last_at_most(n, (int)blockIdx.x, [&](int i) { return (int)recs[i].first_block; });
    const PlaneRec rec = recs[r];
    const VKX_GLOBAL(uint8_t) *src = (const VKX_GLOBAL(uint8_t) *)rec.src;
    VKX_GLOBAL(uint8_t) *dst = (VKX_GLOBAL(uint8_t) *)rec.dst;
    const unsigned begin = (blockIdx.x - rec.first_block) * kPlaneBlockBytes;               // a multiple of 16
    const unsigned end = rec.bytes - begin < kPlaneBlockBytes ? rec.bytes : begin + kPlaneBlockBytes;
    if ((((uintptr_t)rec.src | (uintptr_t)rec.dst) & 15) == 0) {
        words4 v[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const unsigned o = begin + (k * kBlock + threadIdx.x) * 16;
            if (o + 16 <= end) v[k] = *(const VKX_GLOBAL(words4) *)(src + o);
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const unsigned o = begin + (k * kBlock + threadIdx.x) * 16;
            if (o + 16 <= end) *(VKX_GLOBAL(words4) *)(dst + o) = v[k];
        }
        const unsigned whole = end & ~15u;                      // (the last workgroup of the record: its bytes past the last 16)
        if (threadIdx.x < end - whole) dst[whole + threadIdx.x] = src[whole + threadIdx.x];
    } else {
        for (unsigned o = begin + threadIdx.x; o < end; o += kBlock) dst[o] = src[o];
    }
}

template <int kDtype>
void launch_images(hipStream_t stream, dim3 grid, bool planar, const vkx_collate_image *images, const ImageParams &p)
{
    if (planar) k_collate_images<kDtype, true><<<grid, kBlock, 0, stream>>>(images, p);
    else k_collate_images<kDtype, false><<<grid, kBlock, 0, stream>>>(images, p);
}

}  // namespace

VKX_EXPORT int vkx_collate_dev(vkx_ctx *ctx, const vkx_collate_image *images_host, int n_images, const vkx_collate_plane *planes_host,
                               int n_planes, const vkx_collate_norm *norm)
{
    VKX_REQUIRE(ctx != nullptr, "ctx is NULL");
    VKX_REQUIRE(n_images >= 0 && n_images <= kMaxImages, "0 .. 65535 images");
    VKX_REQUIRE(n_planes >= 0 && n_planes <= kMaxPlanes, "0 .. 2^20 planes");
    VKX_REQUIRE((images_host && norm) || n_images == 0, "images without their table or their norm");
    VKX_REQUIRE(planes_host || n_planes == 0, "planes without their table");

    // every destination, then every source against them
    std::vector<std::pair<long long, long long>> dsts, srcs;
    size_t pixels = 0;
    if (n_images) {
        VKX_REQUIRE(norm->height >= 1 && norm->height <= kMaxSide && norm->width >= 1 && norm->width <= kMaxSide, "a side outside 1 .. 32768");
        VKX_REQUIRE(norm->dtype >= VKX_COLLATE_U8 && norm->dtype <= VKX_COLLATE_BF16, "unknown dtype");
        VKX_REQUIRE(norm->channels_first == 0 || norm->channels_first == 1, "channels_first is 0 or 1");
        VKX_REQUIRE(norm->dst != nullptr, "NULL destination");
        const size_t esz = norm->dtype == VKX_COLLATE_U8 ? 1 : (norm->dtype == VKX_COLLATE_F32 ? 4 : 2);
        VKX_REQUIRE((uintptr_t)norm->dst % esz == 0, "the destination is not aligned to its element");
        for (int c = 0; c < 3; c++) VKX_REQUIRE(std::isfinite(norm->mean[c]) && std::isfinite(norm->scale[c]), "mean and scale are finite");
        pixels = (size_t)norm->height * norm->width;
        dsts.push_back({(long long)(uintptr_t)norm->dst, (long long)((uintptr_t)norm->dst + (size_t)n_images * 3 * pixels * esz)});
        for (int i = 0; i < n_images; i++) {
            VKX_REQUIRE(images_host[i].src != nullptr, "NULL source");
            srcs.push_back({(long long)(uintptr_t)images_host[i].src, (long long)((uintptr_t)images_host[i].src + 3 * pixels)});
        }
    }
    long long blocks = 0;
    for (int i = 0; i < n_planes; i++) {
        const vkx_collate_plane &p = planes_host[i];
        VKX_REQUIRE(p.src && p.dst, "NULL plane");
        VKX_REQUIRE(p.bytes >= 1 && p.bytes < ((size_t)1 << 31), "a plane of 1 .. 2^31 - 1 bytes");
        dsts.push_back({(long long)(uintptr_t)p.dst, (long long)((uintptr_t)p.dst + p.bytes)});
        srcs.push_back({(long long)(uintptr_t)p.src, (long long)((uintptr_t)p.src + p.bytes)});
        blocks += (long long)vkx_blocks(p.bytes, kPlaneBlockBytes);
    }
    VKX_REQUIRE(blocks <= INT_MAX, "the planes of one call take fewer than 2^31 workgroups");
    VKX_REQUIRE(!vkx_ranges_overlap(dsts), "two destinations overlap");          // (sorts them)
    for (const auto &s : srcs) {
        // the first destination that ends past the source's start
        auto it = std::upper_bound(dsts.begin(), dsts.end(), s.first,
                                   [](long long at, const std::pair<long long, long long> &d) { return at < d.second; });
        VKX_REQUIRE(it == dsts.end() || it->first >= s.second, "a destination overlaps a source");
    }
    if (n_images == 0 && n_planes == 0) return VKX_OK;

    int rc;
    vkx_tables tab(ctx);
    const size_t img_off = tab.add(sizeof(vkx_collate_image) * (size_t)n_images), rec_off = tab.add(sizeof(PlaneRec) * (size_t)n_planes);
    if ((rc = tab.take())) return rc;
    if (n_images) memcpy(tab.at<vkx_collate_image>(img_off), images_host, sizeof(vkx_collate_image) * (size_t)n_images);
    unsigned first = 0;
    for (int i = 0; i < n_planes; i++) {
        const vkx_collate_plane &p = planes_host[i];
        tab.at<PlaneRec>(rec_off)[i] = PlaneRec{(const uint8_t *)p.src, (uint8_t *)p.dst, (unsigned)p.bytes, first};
        first += vkx_blocks(p.bytes, kPlaneBlockBytes);
    }
    if ((rc = tab.copy_to(&ctx->collate_tables, (size_t)64 << 10))) return rc;      // grows (and syncs) rarely
    const char *base = (const char *)ctx->collate_tables.ptr;
    if (n_images) {
        ImageParams p;
        p.dst = norm->dst;
        p.pixels = (unsigned)pixels;
        for (int c = 0; c < 3; c++) { p.mean[c] = norm->mean[c]; p.scale[c] = norm->scale[c]; }
        const dim3 grid(vkx_blocks(pixels >> 2, kGroupsPerBlock), n_images);
        const vkx_collate_image *images = (const vkx_collate_image *)(base + img_off);
        const bool planar = norm->channels_first != 0;
        VKX_TIMED(ctx, "k_collate_images");
        switch (norm->dtype) {
        case VKX_COLLATE_U8: launch_images<VKX_COLLATE_U8>(ctx->stream, grid, planar, images, p); break;
        case VKX_COLLATE_F32: launch_images<VKX_COLLATE_F32>(ctx->stream, grid, planar, images, p); break;
        case VKX_COLLATE_F16: launch_images<VKX_COLLATE_F16>(ctx->stream, grid, planar, images, p); break;
        default: launch_images<VKX_COLLATE_BF16>(ctx->stream, grid, planar, images, p); break;
        }
    }
    VKX_LAUNCH_CHECK();
    if (n_planes) {
        VKX_TIMED(ctx, "k_collate_planes");
        k_collate_planes<<<first, kBlock, 0, ctx->stream>>>((const PlaneRec *)(base + rec_off), n_planes);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
