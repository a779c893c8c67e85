// The combiner image engine on gfx950 (reference: engine/image/combiner.py:178-333, synthesize_image).
//
// The reference copies texture tiles into a page on the host, marks a band around every tile edge in a mask, blurs the
// whole page with cv.GaussianBlur and keeps the blur on the band only.  Here the host hands over the tile rectangles and
// the page is written by ONE launch: a workgroup owns a 64 x 16 block of the page, gathers the block's window of the mosaic
// (the block and the blur's halo, BORDER_REFLECT_101 at the page border) from the cached textures into LDS once, and every
// lane writes its pixel -- the 8.8 fixed-point separable blur of the window where the pixel lies on a band, the window's
// centre everywhere else.  No intermediate page, no second launch, no atomics.
//
// The tile table is binned on the host into the blocks (vkb::TileBins of vkx_tile_bins.h): a block lists, in table order,
// the tiles whose rectangle widened by max(half, ksize / 2) meets it -- every tile that can cover a pixel of its window or
// put it on a band.  A lane walks that list backwards for the covering tile (the later tile wins) and forwards for the band.
// The first 32 records of a block's list are staged in LDS; a lane resolves the addresses of all its window pixels from them
// before it loads any texture byte, so its loads are in flight together.
//
// LDS: one dword per window pixel (r | g << 8 | b << 16), (16 + ksize - 1) x (64 + ksize - 1) of them -- 9 360 bytes at the
// cap ksize = 15, 5 440 at the reference's 5: occupancy stays bound by the 256-lane workgroup, not by LDS.  A dword per pixel
// keeps a row of lanes on consecutive banks in both passes (a 3-byte interleaved window would put four lanes on three
// banks and split every pixel read in two).  The kernel moves the bytes of a page copy plus the halo, but it is bound by
// instruction issue (address work per window pixel), not by those bytes: DESIGN.md, 'Image combiner'.
#include "vkx_internal.h"
#include "vkx_tile_bins.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kBlockW = 64, kBlockH = 16;
constexpr int kMaxKsize = 15, kMaxHalf = 64;
constexpr long long kMaxEntries = 1ll << 26;    // (block, tile) pairs of one call: 256 MB of table at most
constexpr int kWinCap = (kBlockH + kMaxKsize - 1) * (kBlockW + kMaxKsize - 1);

struct CombineTile {          // a tile as the kernel reads it: the rectangle (inclusive) and its texture
    int up, down, left, right;
    const uint8_t *src;       // dense [*, sw, 3]
    int sw, reserved;
};
static_assert(sizeof(CombineTile) == 32, "CombineTile layout");

struct CombineKernel {
    uint16_t k[kMaxKsize + 1];   // unsigned 8.8 fixed point, sums to 256
    int ksize, half;
};

typedef uint32_t combine_u32_u1 __attribute__((aligned(1)));

// The first kLdsTiles records of a block's list are staged in LDS (a block of a planned page meets a handful of tiles); a longer
// list reads its tail from the table.
constexpr int kLdsTiles = 32;
constexpr int kGather = (kWinCap + 255) / 256;      // window pixels a lane gathers at most

// grid (blocks of 64 columns, blocks of 16 rows); lane = column, 4 rows a wavefront
__global__ void __launch_bounds__(256) k_image_combine(const int *__restrict__ bin_start, const int *__restrict__ bin_items,
                                                       const CombineTile *__restrict__ tiles, CombineKernel K,
                                                       uint8_t *__restrict__ dst, int h, int w)
{
    __shared__ uint32_t win[kWinCap];
    __shared__ CombineTile staged[kLdsTiles];
    const int bin = blockIdx.y * gridDim.x + blockIdx.x;
    const int b0 = bin_start[bin], n_list = bin_start[bin + 1] - b0;
    const int r = K.ksize / 2;
    const int ww = kBlockW + 2 * r, wh = kBlockH + 2 * r;
    const int x0 = blockIdx.x * kBlockW, y0 = blockIdx.y * kBlockH;
    if ((int)threadIdx.x < min(n_list, kLdsTiles)) staged[threadIdx.x] = tiles[bin_items[b0 + threadIdx.x]];
    __syncthreads();
    auto tile_at = [&](int j) -> CombineTile { return j < kLdsTiles ? staged[j] : tiles[bin_items[b0 + j]]; };

    // the window of the mosaic: zeros, then every tile in table order -- the last tile covering a pixel.  The addresses of a
    // lane's pixels are found first (list walks in LDS), then all its texture loads are in flight together.
    const uint8_t *from[kGather];
#pragma unroll
    for (int k = 0; k < kGather; k++) {
        const int i = threadIdx.x + k * 256;
        from[k] = nullptr;
        if (i < ww * wh) {
            const int wy = i / ww, wx = i - wy * ww;
            const int py = vkd::reflect101(y0 - r + wy, h), px = vkd::reflect101(x0 - r + wx, w);
            for (int j = n_list - 1; j >= 0; j--) {
                const CombineTile T = tile_at(j);
                if (py >= T.up && py <= T.down && px >= T.left && px <= T.right) {
                    from[k] = T.src + ((size_t)(py - T.up) * T.sw + (px - T.left)) * 3;
                    break;
                }
            }
        }
    }
    uint32_t got[kGather];
#pragma unroll
    for (int k = 0; k < kGather; k++) {
        got[k] = 0;
        if (from[k]) got[k] = (uint32_t)from[k][0] | ((uint32_t)from[k][1] << 8) | ((uint32_t)from[k][2] << 16);
    }
#pragma unroll
    for (int k = 0; k < kGather; k++) {
        const int i = threadIdx.x + k * 256;
        if (i < ww * wh) win[i] = got[k];
    }
    __syncthreads();

    const int lx = threadIdx.x & 63, x = x0 + lx;
    const int half = K.half;
    for (int ly = threadIdx.x >> 6; ly < kBlockH; ly += 4) {
        const int y = y0 + ly;
        const bool inside = x < w && y < h;
        // fill_np_edge_mask: the rows around a tile's upper and lower edge over its columns, the columns around its left and
        // right edge over its rows (the page clips them: the pixel is inside the page)
        bool edge = false;
        if (inside) {
            for (int j = 0; j < n_list && !edge; j++) {
                const CombineTile T = tile_at(j);
                if (x >= T.left && x <= T.right && (abs(y - T.up) <= half || abs(y - T.down) <= half)) edge = true;
                if (y >= T.up && y <= T.down && (abs(x - T.left) <= half || abs(x - T.right) <= half)) edge = true;
            }
        }
        uint32_t px = win[(ly + r) * ww + lx + r];
        if (edge) {
            // horizontal u8 x 8.8 -> 8.8, then vertical 8.8 x 8.8 -> 16.16, (v + 2^15) >> 16: the arithmetic of k_gaussian_blur
            uint32_t acc0 = 0, acc1 = 0, acc2 = 0;
            for (int j = 0; j < K.ksize; j++) {
                const uint32_t *row = win + (ly + j) * ww + lx;
                uint32_t h0 = 0, h1 = 0, h2 = 0;
                for (int i = 0; i < K.ksize; i++) {
                    const uint32_t v = row[i], kx = K.k[i];
                    h0 += kx * (v & 255u);
                    h1 += kx * ((v >> 8) & 255u);
                    h2 += kx * (v >> 16);
                }
                const uint32_t ky = K.k[j];
                acc0 += ky * min(h0, 65535u);
                acc1 += ky * min(h1, 65535u);
                acc2 += ky * min(h2, 65535u);
            }
            px = (uint32_t)vkd::clamp_u8((int)((acc0 + 32768u) >> 16)) | ((uint32_t)vkd::clamp_u8((int)((acc1 + 32768u) >> 16)) << 8) |
                 ((uint32_t)vkd::clamp_u8((int)((acc2 + 32768u) >> 16)) << 16);
        }
        // four neighbouring lanes store their 12 bytes as three dwords (every lane of the wavefront takes part in the shuffles)
        const int q = lx & 3, base = (threadIdx.x & 63) - q;
        const uint32_t p0 = (uint32_t)__shfl((int)px, base, 64), p1 = (uint32_t)__shfl((int)px, base + 1, 64);
        const uint32_t p2 = (uint32_t)__shfl((int)px, base + 2, 64), p3 = (uint32_t)__shfl((int)px, base + 3, 64);
        if (y >= h) continue;
        uint8_t *d = dst + ((size_t)y * w + (x - q)) * 3;
        if (x - q + 3 < w) {
            if (q == 0) *(combine_u32_u1 *)d = p0 | (p1 << 24);
            else if (q == 1) *(combine_u32_u1 *)(d + 4) = (p1 >> 8) | (p2 << 16);
            else if (q == 2) *(combine_u32_u1 *)(d + 8) = (p2 >> 16) | (p3 << 8);
        } else if (x < w) {
            d += q * 3;
            d[0] = (uint8_t)px;
            d[1] = (uint8_t)(px >> 8);
            d[2] = (uint8_t)(px >> 16);
        }
    }
}

}  // namespace

VKX_EXPORT int vkx_image_combine_u8c3_dev(vkx_ctx *ctx, const vkx_combine_tile *tiles_host, int n_tiles,
                                          const vkx_combine_source *sources_host, int n_sources, int ksize, int half, double sigma,
                                          uint8_t *dst, int h, int w)
{
    VKX_REQUIRE(ctx && dst && (tiles_host || n_tiles == 0) && (sources_host || n_sources == 0), "NULL argument");
    VKX_REQUIRE(h >= 0 && w >= 0 && h <= (1 << 19) && w <= (1 << 19) && (long long)h * w < (1ll << 29), "bad page shape");
    VKX_REQUIRE(n_tiles >= 0 && n_tiles <= (1 << 22) && n_sources >= 0 && n_sources <= (1 << 20), "too many tiles or sources");
    VKX_REQUIRE(ksize >= 1 && (ksize & 1) && ksize <= kMaxKsize, "ksize is odd and in 1 .. 15");
    VKX_REQUIRE(half >= 0 && half <= kMaxHalf, "band half width in 0 .. 64");
    VKX_REQUIRE(std::isfinite(sigma) && sigma > 0, "sigma is finite and positive");
    const size_t dst_bytes = (size_t)h * w * 3;
    for (int i = 0; i < n_sources; i++) {
        const vkx_combine_source &s = sources_host[i];
        VKX_REQUIRE(s.image, "NULL source");
        VKX_REQUIRE(s.height >= 1 && s.width >= 1 && s.height <= (1 << 20) && s.width <= (1 << 20), "bad source shape");
        VKX_REQUIRE(!vkx_planes_overlap(s.image, 1, 0, (size_t)s.height * s.width * 3, dst, 1, 0, dst_bytes),
                    "source and destination overlap");
    }
    for (int i = 0; i < n_tiles; i++) {
        const vkx_combine_tile &t = tiles_host[i];
        VKX_REQUIRE(t.up >= 0 && t.up <= t.down && t.down < h && t.left >= 0 && t.left <= t.right && t.right < w, "tile outside the page");
        VKX_REQUIRE(t.source >= 0 && t.source < n_sources, "source index out of range");
        const vkx_combine_source &s = sources_host[t.source];
        VKX_REQUIRE(t.down - t.up + 1 <= s.height && t.right - t.left + 1 <= s.width, "tile larger than its source");
    }
    if (h == 0 || w == 0) return VKX_OK;
    CombineKernel K;
    memset(&K, 0, sizeof(K));
    K.ksize = ksize;
    K.half = half;
    if (vkx_gaussian_kernel_q8_host(ksize, sigma, K.k)) {
        vkx_set_error("%s: no 8.8 kernel for ksize=%d sigma=%g", __func__, ksize, sigma);
        return VKX_ERR_INVALID;
    }

    // bin the tiles into the blocks their widened rectangle meets (table order inside a block); refused while the pairs are
    // counted, before the counting (and the filling) can run long
    const int reach = std::max(half, ksize / 2);
    vkb::TileBins<kBlockW, kBlockH> bins(h, w);
    auto span_of = [&](int i) {
        const vkx_combine_tile &t = tiles_host[i];
        return bins.rect(std::max(0, t.up - reach), std::min(h - 1, t.down + reach), std::max(0, t.left - reach),
                         std::min(w - 1, t.right + reach));
    };
    VKX_REQUIRE(bins.count(n_tiles, kMaxEntries - 1, span_of), "tile table too large for its page");
    vkx_tables tab(ctx);
    const size_t off_start = tab.add(sizeof(int) * bins.start.size());
    const size_t off_items = tab.add(sizeof(int) * std::max<size_t>(bins.pairs(), 1));
    const size_t off_tiles = tab.add(sizeof(CombineTile) * (size_t)std::max(n_tiles, 1));
    int rc = tab.take();
    if (rc) return rc;
    memcpy(tab.at<int>(off_start), bins.start.data(), sizeof(int) * bins.start.size());
    bins.fill(n_tiles, tab.at<int>(off_items), span_of);
    CombineTile *recs = tab.at<CombineTile>(off_tiles);
    for (int i = 0; i < n_tiles; i++) {
        const vkx_combine_tile &t = tiles_host[i];
        recs[i] = CombineTile{t.up, t.down, t.left, t.right, sources_host[t.source].image, sources_host[t.source].width, 0};
    }
    if ((rc = tab.copy_to(&ctx->combine_tables, (size_t)256 << 10))) return rc;   // grows (and syncs) rarely
    const unsigned char *base = (const unsigned char *)ctx->combine_tables.ptr;
    dim3 grid(bins.tiles_x, bins.tiles_y);
    {
        VKX_TIMED(ctx, "k_image_combine");
        k_image_combine<<<grid, 256, 0, ctx->stream>>>((const int *)(base + off_start), (const int *)(base + off_items),
                                                       (const CombineTile *)(base + off_tiles), K, dst, h, w);
    }
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
