// jpeg_quality (reference photometric/effect.py:41-42): cv.imdecode(cv.imencode('.jpeg', mat, [IMWRITE_JPEG_QUALITY, q]))
// as libjpeg-turbo computes it.  Entropy coding is lossless, so for a fixed quality the round trip is
//   RGB -> YCbCr (16-bit fixed point) -> h2v2 downsampling (bias 1, 2 alternating along a row) -> 8x8 accurate integer FDCT
//   (CONST_BITS 13, PASS1_BITS 2) -> quantise (round half away from zero of coef / 8q) -> dequantise -> accurate integer IDCT
//   (its RANGE_MASK sample table) -> h2v2 fancy upsampling (3:1, +8 / +7; plain replication when the chroma plane is at
//   most 2 samples wide) -> YCbCr -> RGB.
// A 3-channel mat is BGR to the codec: channel 2 carries the R weight.  A 1-channel mat is a one-component JPEG (luma table).
// Edges: luma blocks replicate the last column / row; chroma takes the right edge by input columns before the 2 x 2 sums and
// the bottom edge by repeating the last downsampled row.  tests/jpeg_restate.py is the statement the goldens of the library pin.
//
// Launch 1 (k_jpeg_blocks): 32 blocks of one plane per workgroup, one thread per (block, row): the row passes run in
// registers, rows and columns are exchanged through LDS (block stride 65 words: no bank conflicts).  It writes the decoded
// planes at their padded sizes into ctx->jpeg_planes, or, for one channel, the cropped result straight into dst.
// Launch 2 (k_jpeg_upsample): one thread per chroma sample: the 2 x 2 output pixels it feeds, from its 3 x 3 neighbourhood.
#include "vkx_internal.h"
#include "vkx_jpeg.h"

namespace {

constexpr int kBlocksPerGroup = 32;
constexpr int kLdsStride = 65;

using namespace vkx_jpeg;      // the tables, colour conversion and forward DCT pass shared with jpeg_encode.hip

// one pass of the inverse DCT over d[0..7]; `last`: the row pass (descale by CONST_BITS + PASS1_BITS + 3)
template <bool last>
__device__ __forceinline__ void idct8(int *d)
{
    constexpr int sh = last ? 13 + 2 + 3 : 13 - 2;
    const int z1e = (d[2] + d[6]) * C_0_541;
    const int e2 = z1e - d[6] * C_1_847, e3 = z1e + d[2] * C_0_765;
    const int e0 = (d[0] + d[4]) * 8192, e1 = (d[0] - d[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    const int o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
    const int z5 = (o0 + o2 + o1 + o3) * C_1_175;
    const int z1 = -(o0 + o3) * C_0_899, z2 = -(o1 + o2) * C_2_562;
    const int z3 = -(o0 + o2) * C_1_961 + z5, z4 = -(o1 + o3) * C_0_390 + z5;
    const int p0 = o0 * C_0_298 + z1 + z3, p1 = o1 * C_2_053 + z2 + z4;
    const int p2 = o2 * C_3_072 + z2 + z3, p3 = o3 * C_1_501 + z1 + z4;
    d[0] = descale(t10 + p3, sh);
    d[7] = descale(t10 - p3, sh);
    d[1] = descale(t11 + p2, sh);
    d[6] = descale(t11 - p2, sh);
    d[2] = descale(t12 + p1, sh);
    d[5] = descale(t12 - p1, sh);
    d[3] = descale(t13 + p0, sh);
    d[4] = descale(t13 - p0, sh);
}

// the post-IDCT sample table indexed by value & RANGE_MASK (1023): clamp(v + 128) on [-512, 512), wrapping beyond
__device__ __forceinline__ int range_limit(int v)
{
    v &= 1023;
    v -= (v & 512) << 1;
    return min(max(v + 128, 0), 255);
}

// plane 0: Y (or the single channel), 1: Cb, 2: Cr.  Blocks of a plane are numbered row-major; workgroups [base[p], base[p+1])
// take plane p.
struct BlockGrid {
    int base[4];        // first workgroup of each plane; base[3]: the grid size
    int bw[3];          // blocks per row
    int nblk[3];        // blocks in the plane
    int pitch[3];       // bytes per row of the decoded plane (padded width)
    size_t off[3];      // the decoded plane inside the scratch
};

template <int CN>
__global__ void __launch_bounds__(256) k_jpeg_blocks(const uint8_t *__restrict__ src, int h, int w, ptrdiff_t src_stride,
                                                     uint8_t *__restrict__ planes, uint8_t *__restrict__ dst, ptrdiff_t dst_stride,
                                                     BlockGrid g, JpegTables t)
{
    __shared__ int lds[kBlocksPerGroup * kLdsStride];
    const int wg = blockIdx.x;
    const int plane = wg >= g.base[2] ? 2 : wg >= g.base[1] ? 1 : 0;      // uniform over the workgroup
    const int r = threadIdx.x >> 5, b = threadIdx.x & 31;                  // row of the block, block of the group
    const int blk = (wg - g.base[plane]) * kBlocksPerGroup + b;
    const bool live = blk < g.nblk[plane];
    const int by = live ? blk / g.bw[plane] : 0, bx = live ? blk - by * g.bw[plane] : 0;
    const int tab = plane ? 1 : 0;

    int d[8];
    if (plane == 0) {
        const uint8_t *row = src + (size_t)min(by * 8 + r, h - 1) * src_stride;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint8_t *p = row + (size_t)min(bx * 8 + k, w - 1) * CN;
            d[k] = (CN == 1 ? (int)p[0] : rgb_y(p[2], p[1], p[0])) - 128;
        }
    } else {
        const int dh = (h + 1) >> 1;
        const int cy = min(by * 8 + r, dh - 1);
        const uint8_t *row0 = src + (size_t)(2 * cy) * src_stride;
        const uint8_t *row1 = src + (size_t)min(2 * cy + 1, h - 1) * src_stride;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cx = bx * 8 + k;
            const size_t x0 = (size_t)min(2 * cx, w - 1) * CN, x1 = (size_t)min(2 * cx + 1, w - 1) * CN;
            const uint8_t *px[4] = {row0 + x0, row0 + x1, row1 + x0, row1 + x1};
            int s = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                s += plane == 1 ? rgb_cb(px[i][2], px[i][1], px[i][0]) : rgb_cr(px[i][2], px[i][1], px[i][0]);
            d[k] = ((s + 1 + (k & 1)) >> 2) - 128;
        }
    }

    // rows: forward pass 1, then to LDS
    fdct8<false>(d);
    int *mine = lds + b * kLdsStride;
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[r * 8 + k] = d[k];
    __syncthreads();
    // column c = r: forward pass 2, quantise, dequantise, inverse pass 1
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = mine[k * 8 + r];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int qv = t.q[tab][k * 8 + r];
        const int a = abs(d[k]);
        const int mag = (int)__umulhi((unsigned)(a + 4 * qv), t.m[tab][k * 8 + r]);
        d[k] = (d[k] < 0 ? -mag : mag) * qv;
    }
    idct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[k * 8 + r] = d[k];      // the column this thread read: no other thread touches it
    __syncthreads();
    // rows: inverse pass 2, range limit, store
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = mine[r * 8 + k];
    idct8<true>(d);
    if (!live) return;
    if (CN == 1) {
        const int y = by * 8 + r;
        if (y >= h) return;
        uint8_t *out = dst + (size_t)y * dst_stride + bx * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (bx * 8 + k < w) out[k] = (uint8_t)range_limit(d[k]);
        return;
    }
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= (uint32_t)range_limit(d[k]) << (8 * k);
        hi |= (uint32_t)range_limit(d[k + 4]) << (8 * k);
    }
    // padded planes: rows of whole blocks, 8-byte aligned
    uint2 *out = (uint2 *)(planes + g.off[plane] + (size_t)(by * 8 + r) * g.pitch[plane] + bx * 8);
    *out = make_uint2(lo, hi);
}

__device__ __forceinline__ int fancy(int c, int n, int odd) { return (3 * c + n + 8 - odd) >> 4; }

__global__ void __launch_bounds__(256) k_jpeg_upsample(const uint8_t *__restrict__ planes, BlockGrid g, int h, int w,
                                                       uint8_t *__restrict__ dst, ptrdiff_t dst_stride)
{
    const int dh = (h + 1) >> 1, dw = (w + 1) >> 1;
    const int cx = blockIdx.x * 64 + (threadIdx.x & 63), cy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx >= dw || cy >= dh) return;
    const uint8_t *Y = planes + g.off[0];
    int cb[2][2], cr[2][2];     // [output row parity][output column parity]
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint8_t *C = planes + g.off[1 + p];
        const int pitch = g.pitch[1 + p];
        int v[2][2];
        if (dw <= 2) {      // the library does not fancy-upsample a plane this narrow: replication
            v[0][0] = v[0][1] = v[1][0] = v[1][1] = C[(size_t)cy * pitch + cx];
        } else {
            const int rows[3] = {max(cy - 1, 0), cy, min(cy + 1, dh - 1)};
            const int cols[3] = {max(cx - 1, 0), cx, min(cx + 1, dw - 1)};
            int s[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) s[i][j] = C[(size_t)rows[i] * pitch + cols[j]];
#pragma unroll
            for (int vy = 0; vy < 2; ++vy) {
                int cs[3];      // column sums towards the upper (vy 0) or lower (vy 1) neighbour row
#pragma unroll
                for (int j = 0; j < 3; ++j) cs[j] = 3 * s[1][j] + s[vy ? 2 : 0][j];
                v[vy][0] = fancy(cs[1], cs[0], 0);
                v[vy][1] = fancy(cs[1], cs[2], 1);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) (p ? cr : cb)[i][j] = v[i][j];
    }
#pragma unroll
    for (int vy = 0; vy < 2; ++vy) {
        const int y = 2 * cy + vy;
        if (y >= h) break;
        uint8_t *out = dst + (size_t)y * dst_stride;
#pragma unroll
        for (int vx = 0; vx < 2; ++vx) {
            const int x = 2 * cx + vx;
            if (x >= w) break;
            const int yy = Y[(size_t)y * g.pitch[0] + x];
            const int xb = cb[vy][vx] - 128, xr = cr[vy][vx] - 128;
            const int rr = yy + ((91881 * xr + 32768) >> 16);
            const int gg = yy + ((-22554 * xb + 32768 - 46802 * xr) >> 16);
            const int bb = yy + ((116130 * xb + 32768) >> 16);
            uint8_t *o = out + (size_t)x * 3;
            o[0] = (uint8_t)min(max(bb, 0), 255);
            o[1] = (uint8_t)min(max(gg, 0), 255);
            o[2] = (uint8_t)min(max(rr, 0), 255);
        }
    }
}

} // namespace

VKX_EXPORT int vkx_jpeg_roundtrip_u8_dev(vkx_ctx *ctx, const uint8_t *src, int h, int w, int cn, ptrdiff_t src_stride,
                                         uint8_t *dst, ptrdiff_t dst_stride, int quality)
{
    VKX_REQUIRE_PITCH(src_stride, (ptrdiff_t)w * cn, h);
    VKX_REQUIRE_PITCH(dst_stride, (ptrdiff_t)w * cn, h);
    VKX_REQUIRE_DISJOINT(src, h, src_stride, (ptrdiff_t)w * cn, dst, h, dst_stride, (ptrdiff_t)w * cn);
    VKX_REQUIRE(ctx && src && dst, "NULL argument");
    VKX_REQUIRE(h > 0 && w > 0 && h <= (1 << 28) / 8 && w <= (1 << 28) / 8, "bad shape");
    VKX_REQUIRE(cn == 1 || cn == 3, "1 or 3 channels");
    VKX_REQUIRE(0 <= quality && quality <= 100, "quality in 0 .. 100");
    VKX_REQUIRE(src_stride >= (ptrdiff_t)w * cn && dst_stride >= (ptrdiff_t)w * cn, "stride below the row");
    const JpegTables t = jpeg_tables(quality);

    BlockGrid g = {};
    const int np = cn == 1 ? 1 : 3;
    const int ph[3] = {(h + 7) / 8, ((h + 1) / 2 + 7) / 8, ((h + 1) / 2 + 7) / 8};
    const int pw[3] = {(w + 7) / 8, ((w + 1) / 2 + 7) / 8, ((w + 1) / 2 + 7) / 8};
    size_t bytes = 0;
    long groups = 0;
    for (int p = 0; p < 3; ++p) {
        g.base[p] = (int)groups;
        if (p >= np) continue;
        g.bw[p] = pw[p];
        g.nblk[p] = ph[p] * pw[p];
        g.pitch[p] = pw[p] * 8;
        g.off[p] = bytes;
        bytes += (size_t)ph[p] * 8 * g.pitch[p];
        groups += (g.nblk[p] + kBlocksPerGroup - 1) / kBlocksPerGroup;
    }
    VKX_REQUIRE(groups < INT_MAX, "image too large");
    for (int p = np; p < 3; ++p) g.base[p] = (int)groups;
    g.base[3] = (int)groups;

    uint8_t *planes = nullptr;
    if (cn == 3) {
        int rc = vkx_scratch_reserve(ctx, &ctx->jpeg_planes, bytes);
        if (rc) return rc;
        planes = (uint8_t *)ctx->jpeg_planes.ptr;
    }
    {
        VKX_TIMED(ctx, "k_jpeg_blocks");
        if (cn == 1)
            k_jpeg_blocks<1><<<(unsigned)groups, 256, 0, ctx->stream>>>(src, h, w, src_stride, planes, dst, dst_stride, g, t);
        else
            k_jpeg_blocks<3><<<(unsigned)groups, 256, 0, ctx->stream>>>(src, h, w, src_stride, planes, dst, dst_stride, g, t);
        VKX_LAUNCH_CHECK();
    }
    if (cn == 1) return VKX_OK;
    VKX_TIMED(ctx, "k_jpeg_upsample");
    dim3 grid(vkx_blocks((size_t)(w + 1) / 2, 64), vkx_blocks((size_t)(h + 1) / 2, 4));
    k_jpeg_upsample<<<grid, 256, 0, ctx->stream>>>(planes, g, h, w, dst, dst_stride);
    VKX_LAUNCH_CHECK();
    return VKX_OK;
}
