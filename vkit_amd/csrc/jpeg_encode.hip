// Image.to_file / to_pil_image().save (reference image.py:351-359) for JPEG, on gfx950: a batch of dense uint8 images into the
// files Pillow's libjpeg-turbo writes with its defaults -- JFIF 1.1, baseline, 4:2:0 for three channels, one component for one,
// the Annex K Huffman tables, no restart markers --, byte for byte, packed back to back (include/vkx.h, "JPEG encode").
// tests/jpeg_encode_restate.py is the statement the goldens pin.  The lossy half is jpeg.hip's (vkx_jpeg.h); the lossless half
// is the part with sequential dependencies -- DC prediction, bit offsets, stuffing offsets -- and is cut into launches so that
// every dependency is either inside one workgroup or between two launches.  No workgroup ever waits for another.
//
//   1 k_enc_coef         32 blocks a workgroup, one thread per (block, row) as k_jpeg_blocks: colour conversion, h2v2 downsampling,
//                        FDCT, quantiser; int16 coefficients in zigzag order, each block at its place in SCAN order (colour: per
//                        16 x 16 MCU Y00 Y01 Y10 Y11 Cb Cr; grey: row-major), libjpeg's dummy blocks included: a dummy is the
//                        DC of the real block compress_data copies it from (found by arithmetic, transformed again) and zero AC.
//   2 k_enc_lengths      one wavefront per block, one lane per zigzag position.  A 64-bit ballot of the non-zero AC positions
//                        gives a lane its run (distance to the set bit below it), its ZRL count and symbol; lane 0 codes the DC
//                        difference against the previous block of its component in scan order (an index, read from the
//                        coefficients); lane 63 codes the EOB when coefficient 63 is zero.  The wave sum of the code lengths
//                        is the block's bit count.
//   3 k_enc_scan_blocks  one workgroup per image walks its blocks a round at a time (128, or 8192 where an image has more than
//                        2048): exclusive scan of the bit counts (64-bit).
//   4 k_enc_pack         the wave shape of 2: a lane ORs its at most 59 bits (three ZRL of 11, a 16-bit code, 10 magnitude
//                        bits) into the zeroed big-endian bit stream of its image with atomicOr on 32-bit words; the wave of
//                        an image's last block pads the last byte with 1-bits (flush_bits).
//   5 k_enc_count_ff     the 0xFF bytes of every 2048-byte chunk of the unstuffed streams.
//   6 k_enc_scan_chunks  one workgroup per image: exclusive scan of its chunks' counts; the image's file size.
//   7 k_enc_offsets      one workgroup: exclusive scan of the file sizes into `offsets`.
//   8 k_enc_assemble     a workgroup per chunk scatters its bytes behind the image's header with a 0x00 after every 0xFF; the
//                        first chunk's workgroup copies the header (built on the host, staged with the tables) and writes EOI.
//                        Every store is bounded by `capacity`.
// The unstuffed stream of an image is given the proven bound of 208 bytes a block ((9 + 11) + 63 * (16 + 10) bits for luma; chroma's
// DC category 11 has an 11-bit code: 1660 bits), so its place is known before anything is coded: 20 MB for a 2048^2 RGB page
// (98 304 blocks), next to 12 MB of coefficients.
#include "vkx_internal.h"
#include "vkx_jpeg.h"

#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace {

using namespace vkx_jpeg;

constexpr int kBlocksPerGroup = 32;
constexpr int kLdsStride = 65;
constexpr int kMaxImages = 65535, kMaxSide = 32768;
constexpr unsigned kMaxBlocks = 1u << 26;            // of one call: block indices, bit counts and grids stay far inside their types
constexpr unsigned kBlockBytes = 208;                // the unstuffed stream of a block never takes more
constexpr unsigned kChunkBytes = 2048;               // of the unstuffed stream, a workgroup of the stuffing launches (8 bytes a lane)
constexpr int kHuffStride = 16 + 256;                // a table pair: DC by category, then AC by symbol; (code << 8) | length

struct ImgRec {
    const uint8_t *src;
    int h, w, cn;
    int ybw, ybh;                 // luma (or grey) blocks a row, rows of them
    int mcus_x;                   // colour: MCUs a row
    unsigned nblk, blk0;          // blocks of the scan, dummies included; the first of them among the call's
    unsigned wg0;                 // its first workgroup of k_enc_coef
    unsigned chunk0, nchunks;     // its chunks of the unstuffed stream
    unsigned hdr_off, hdr_len;    // its header inside the staged blob
};

// jpeg_natural_order: zigzag position -> natural index (a constexpr array serves the kernels and the host alike)
constexpr unsigned char kZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_enc_coef(const ImgRec *__restrict__ imgs, int n, int bgr, int16_t *__restrict__ coef,
                                                  JpegTables t)
{
    __shared__ int lds[kBlocksPerGroup * kLdsStride];
    const int img = vkd::last_at_most(n, (int)blockIdx.x, [&](int i) { return (int)imgs[i].wg0; });
    const ImgRec rec = imgs[img];
    const int r = threadIdx.x >> 5, b = threadIdx.x & 31;                  // row of the block, block of the group
    const unsigned s = (blockIdx.x - rec.wg0) * kBlocksPerGroup + b;       // the block in the image's scan order
    const bool live = s < rec.nblk;
    const int h = rec.h, w = rec.w, cn = rec.cn;

    // which block of which plane the scan position holds; a dummy takes the real block its DC is copied from
    int plane = 0, by = 0, bx = 0;
    bool dummy = false;
    if (live) {
        if (cn == 1) {
            by = (int)(s / (unsigned)rec.ybw);
            bx = (int)(s - (unsigned)by * (unsigned)rec.ybw);
        } else {
            const unsigned m = s / 6, k = s - 6 * m;
            const int my = (int)(m / (unsigned)rec.mcus_x), mx = (int)(m - (unsigned)my * (unsigned)rec.mcus_x);
            if (k < 4) {
                by = 2 * my + (int)(k >> 1);
                bx = 2 * mx + (int)(k & 1);
                if (by >= rec.ybh) {            // a missing block row: the DC of the last block of the row above, Y01 (or what stands for it)
                    dummy = true;
                    by = rec.ybh - 1;
                    bx = min(2 * mx + 1, rec.ybw - 1);
                } else if (bx >= rec.ybw) {     // a missing block column: the DC of the block before it
                    dummy = true;
                    bx = rec.ybw - 1;
                }
            } else {
                plane = (int)k - 3;
                by = my;
                bx = mx;
            }
        }
    }
    const int tab = plane ? 1 : 0;
    const int ri = bgr ? 2 : 0, bi = 2 - ri;

    int d[8];
    if (plane == 0) {
        const uint8_t *row = rec.src + (size_t)min(by * 8 + r, h - 1) * ((size_t)w * cn);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint8_t *p = row + (size_t)min(bx * 8 + k, w - 1) * cn;
            d[k] = (cn == 1 ? (int)p[0] : rgb_y(p[ri], p[1], p[bi])) - 128;
        }
    } else {
        const int dh = (h + 1) >> 1;
        const int cy = min(by * 8 + r, dh - 1);
        const uint8_t *row0 = rec.src + (size_t)(2 * cy) * ((size_t)w * 3);
        const uint8_t *row1 = rec.src + (size_t)min(2 * cy + 1, h - 1) * ((size_t)w * 3);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cx = bx * 8 + k;
            const size_t x0 = (size_t)min(2 * cx, w - 1) * 3, x1 = (size_t)min(2 * cx + 1, w - 1) * 3;
            const uint8_t *px[4] = {row0 + x0, row0 + x1, row1 + x0, row1 + x1};
            int sum = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                sum += plane == 1 ? rgb_cb(px[i][ri], px[i][1], px[i][bi]) : rgb_cr(px[i][ri], px[i][1], px[i][bi]);
            d[k] = ((sum + 1 + (k & 1)) >> 2) - 128;
        }
    }

    // rows: forward pass 1, then to LDS; column c = r: forward pass 2, quantise
    fdct8<false>(d);
    int *mine = lds + b * kLdsStride;
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[r * 8 + k] = d[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = mine[k * 8 + r];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int qv = t.q[tab][k * 8 + r];
        const int a = abs(d[k]);
        const int mag = (int)__umulhi((unsigned)(a + 4 * qv), t.m[tab][k * 8 + r]);
        mine[k * 8 + r] = d[k] < 0 ? -mag : mag;      // the column this thread read: no other thread touches it
    }
    __syncthreads();
    // zigzag positions 8r .. 8r + 7 of the block: one 16-byte store
    uint32_t out[4];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        int lo = mine[kZigzag[r * 8 + k]], hi = mine[kZigzag[r * 8 + k + 1]];
        if (dummy) {
            if (r * 8 + k != 0) lo = 0;
            hi = 0;
        }
        out[k >> 1] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
    }
    if (live) *(uint4 *)(coef + ((size_t)rec.blk0 + s) * 64 + r * 8) = make_uint4(out[0], out[1], out[2], out[3]);
}

// ---- launches 2 and 4: a wavefront per block -----------------------------------------------------------------------------------

struct LaneCode {
    uint64_t code;      // at most 59 bits, the first bit of the stream the highest
    unsigned len;
};

// What lane `lane` of a block's wave emits: lane 0 the DC difference `v`, a lane with a non-zero coefficient `v` the ZRLs of
// its run, its symbol and its magnitude bits, lane 63 the EOB when its coefficient is zero.  `acmask`: the non-zero AC positions.
__device__ __forceinline__ LaneCode lane_code(const uint32_t *__restrict__ huff, int lane, int v, uint64_t acmask)
{
    LaneCode c = {0, 0};
    const int a = abs(v);
    const unsigned size = a ? 32u - (unsigned)__clz(a) : 0u;
    const uint64_t magnitude = (uint64_t)((unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u));
    if (lane == 0) {
        const uint32_t e = huff[size];
        c.code = ((uint64_t)(e >> 8) << size) | magnitude;
        c.len = (e & 0xffu) + size;
    } else if (v != 0) {
        const uint64_t below = (acmask | 1ull) & ((1ull << lane) - 1ull);       // bit 0 stands for the DC position
        const int prev = 63 - __clzll((long long)below);
        const unsigned run = (unsigned)(lane - 1 - prev);
        const uint32_t zrl = huff[16 + 0xF0], e = huff[16 + (((run & 15u) << 4) | size)];
        for (unsigned i = 0; i < (run >> 4); ++i) {
            c.code = (c.code << (zrl & 0xffu)) | (zrl >> 8);
            c.len += zrl & 0xffu;
        }
        c.code = (((c.code << (e & 0xffu)) | (e >> 8)) << size) | magnitude;
        c.len += (e & 0xffu) + size;
    } else if (lane == 63) {
        const uint32_t e = huff[16];
        c.code = e >> 8;
        c.len = e & 0xffu;
    }
    return c;
}

__device__ __forceinline__ unsigned wave_inclusive_sum(unsigned x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// The block `gb` of the call as its wave sees it: the image, the block's place in it, and the lane's code.
__device__ __forceinline__ LaneCode wave_block(const ImgRec *__restrict__ imgs, int n, unsigned gb, const int16_t *__restrict__ coef,
                                               const uint32_t *__restrict__ huff, int lane, ImgRec &rec, unsigned &s)
{
    const int img = vkd::last_at_most(n, (int)gb, [&](int i) { return (int)imgs[i].blk0; });
    rec = imgs[img];
    s = gb - rec.blk0;
    int v = coef[(size_t)gb * 64 + lane];
    // the previous block of the same component in scan order
    long long pred = -1;
    int tab = 0;
    if (rec.cn == 1) {
        pred = (long long)s - 1;
    } else {
        const unsigned k = s % 6;
        tab = k >= 4;
        pred = k == 0 ? (long long)s - 3 : (k < 4 ? (long long)s - 1 : (long long)s - 6);
    }
    const uint64_t acmask = __ballot(lane > 0 && v != 0);
    if (lane == 0 && pred >= 0) v -= coef[((size_t)rec.blk0 + (size_t)pred) * 64];
    return lane_code(huff + tab * kHuffStride, lane, v, acmask);
}

__global__ void __launch_bounds__(256) k_enc_lengths(const ImgRec *__restrict__ imgs, int n, unsigned total_blocks,
                                                     const int16_t *__restrict__ coef, const uint32_t *__restrict__ huff,
                                                     uint32_t *__restrict__ blk_bits)
{
    const unsigned gb = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gb >= total_blocks) return;            // (a whole wave)
    ImgRec rec;
    unsigned s;
    const LaneCode c = wave_block(imgs, n, gb, coef, huff, lane, rec, s);
    const unsigned sum = wave_inclusive_sum(c.len, lane);
    if (lane == 63) blk_bits[gb] = sum;
}

// ORs the `len` (<= 59) bits of `code` into the big-endian bit stream `stream` (4-byte aligned, zero where nothing was written
// yet) at bit `at`.  Words that take no set bit are left alone, so nothing past the last coded bit is ever touched.
__device__ __forceinline__ void put_bits(uint8_t *stream, uint64_t at, uint64_t code, unsigned len)
{
    if (!len) return;
    const unsigned o = (unsigned)(at & 31u);
    const unsigned sh = 96u - o - len;                    // the code's last bit above the end of a 96-bit window: 6 .. 95
    uint64_t hi;                                          // bits 95 .. 32 of the window
    uint32_t lo;                                          // bits 31 .. 0
    if (sh >= 32) {
        hi = code << (sh - 32);
        lo = 0;
    } else {
        hi = sh ? code >> (32 - sh) : code >> 32;
        lo = (uint32_t)(code << sh);
    }
    unsigned int *word = (unsigned int *)stream + (at >> 5);
    const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi;
    if (w0) atomicOr(word, __builtin_bswap32(w0));
    if (w1) atomicOr(word + 1, __builtin_bswap32(w1));
    if (lo) atomicOr(word + 2, __builtin_bswap32(lo));
}

__global__ void __launch_bounds__(256) k_enc_pack(const ImgRec *__restrict__ imgs, int n, unsigned total_blocks,
                                                  const int16_t *__restrict__ coef, const uint32_t *__restrict__ huff,
                                                  const uint64_t *__restrict__ blk_off, uint8_t *__restrict__ streams)
{
    const unsigned gb = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gb >= total_blocks) return;
    ImgRec rec;
    unsigned s;
    const LaneCode c = wave_block(imgs, n, gb, coef, huff, lane, rec, s);
    const unsigned sum = wave_inclusive_sum(c.len, lane);
    uint8_t *stream = streams + (size_t)rec.blk0 * kBlockBytes;
    const uint64_t at = blk_off[gb];
    put_bits(stream, at + (sum - c.len), c.code, c.len);
    if (s == rec.nblk - 1 && lane == 63) {               // flush_bits: the last byte filled up with 1-bits
        const uint64_t end = at + sum;
        const unsigned pad = (unsigned)(-(long long)end & 7);
        put_bits(stream, end, (1u << pad) - 1u, pad);
    }
}

// ---- launches 3, 6, 7: scans inside one workgroup ------------------------------------------------------------------------------

// A scan runs in one of two shapes, chosen on the host from the longest range the launch has (scan_is_small): a single wave
// with two entries a lane -- 128 entries a round; a workgroup per image of a batch of small crops would otherwise be sixteen
// waves of which fifteen idle --, or 1024 threads with eight entries each, 8192 a round, for pages.
struct ScanSmall { static constexpr int kThreads = 64, kItems = 2; };
struct ScanLarge { static constexpr int kThreads = 1024, kItems = 8; };
constexpr unsigned kScanSmallMax = 2048;             // the longest range the small shape takes: 16 rounds

// exclusive sum of `v` over the threads of the workgroup, and their total; `lds`: a word per wave
__device__ __forceinline__ uint64_t block_exclusive_sum(uint64_t v, uint64_t *lds, uint64_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) {
        const uint64_t t = lds[i];
        if (i < wave) before += t;
        all += t;
    }
    __syncthreads();            // lds is free again
    total = all;
    return before + x - v;
}

// Exclusive sums of in(0 .. count) handed to out(i, sum), S::kItems consecutive entries a thread and S::kThreads * S::kItems a
// round, the rounds chained by a carry; returns the total (in every thread).
template <class S, class In, class Out>
__device__ __forceinline__ uint64_t scan_range(unsigned count, In in, Out out)
{
    __shared__ uint64_t lds[S::kThreads / 64];
    uint64_t carry = 0;
    for (unsigned base = 0; base < count; base += S::kThreads * S::kItems) {
        const unsigned first = base + threadIdx.x * S::kItems;
        uint64_t v[S::kItems], sum = 0;
#pragma unroll
        for (int k = 0; k < S::kItems; ++k) {
            v[k] = first + k < count ? in(first + k) : 0;
            sum += v[k];
        }
        uint64_t total;
        uint64_t before = carry + block_exclusive_sum(sum, lds, total);
#pragma unroll
        for (int k = 0; k < S::kItems; ++k) {
            if (first + k < count) out(first + k, before);
            before += v[k];
        }
        carry += total;
    }
    return carry;
}

template <class S>
__global__ void __launch_bounds__(S::kThreads) k_enc_scan_blocks(const ImgRec *__restrict__ imgs, const uint32_t *__restrict__ blk_bits,
                                                                 uint64_t *__restrict__ blk_off, uint64_t *__restrict__ img_bits)
{
    const ImgRec rec = imgs[blockIdx.x];
    const uint64_t bits = scan_range<S>(rec.nblk, [&](unsigned i) { return (uint64_t)blk_bits[rec.blk0 + i]; },
                                        [&](unsigned i, uint64_t before) { blk_off[rec.blk0 + i] = before; });
    if (threadIdx.x == 0) img_bits[blockIdx.x] = bits;
}

template <class S>
__global__ void __launch_bounds__(S::kThreads) k_enc_scan_chunks(const ImgRec *__restrict__ imgs, const uint32_t *__restrict__ chunk_ff,
                                                                 const uint64_t *__restrict__ img_bits, uint64_t *__restrict__ chunk_off,
                                                                 uint64_t *__restrict__ img_size)
{
    const ImgRec rec = imgs[blockIdx.x];
    const uint64_t stuffed = scan_range<S>(rec.nchunks, [&](unsigned i) { return (uint64_t)chunk_ff[rec.chunk0 + i]; },
                                           [&](unsigned i, uint64_t before) { chunk_off[rec.chunk0 + i] = before; });
    // header, the stream with its stuffed bytes, EOI
    if (threadIdx.x == 0) img_size[blockIdx.x] = (uint64_t)rec.hdr_len + ((img_bits[blockIdx.x] + 7) >> 3) + stuffed + 2;
}

template <class S>
__global__ void __launch_bounds__(S::kThreads) k_enc_offsets(const uint64_t *__restrict__ img_size, int n, int64_t *__restrict__ offsets)
{
    const uint64_t total = scan_range<S>((unsigned)n, [&](unsigned i) { return img_size[i]; },
                                         [&](unsigned i, uint64_t before) { offsets[i] = (int64_t)before; });
    if (threadIdx.x == 0) offsets[n] = (int64_t)total;
}

// ---- launches 5 and 8: the stuffing ----------------------------------------------------------------------------------------------

// the 8 bytes of this lane in chunk `chunk` of the call: its image, where they start in the image's unstuffed stream, how many
// bytes that stream has; the bytes themselves (zero past the stream's end)
__device__ __forceinline__ uint2 chunk_bytes(const ImgRec *__restrict__ imgs, int n, unsigned chunk, const uint64_t *__restrict__ img_bits,
                                             const uint8_t *__restrict__ streams, int &img, uint64_t &start, uint64_t &bytes)
{
    img = vkd::last_at_most(n, (int)chunk, [&](int i) { return (int)imgs[i].chunk0; });
    const unsigned blk0 = imgs[img].blk0;
    start = (uint64_t)(chunk - imgs[img].chunk0) * kChunkBytes + threadIdx.x * 8u;
    bytes = (img_bits[img] + 7) >> 3;
    // (a group that starts inside the stream lies inside the image's 208 bytes a block: both are multiples of 8)
    return start < bytes ? *(const uint2 *)(streams + (size_t)blk0 * kBlockBytes + start) : make_uint2(0, 0);
}

__device__ __forceinline__ unsigned count_ff(uint2 v)
{
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += (((v.x >> (8 * j)) & 0xffu) == 0xffu) + (((v.y >> (8 * j)) & 0xffu) == 0xffu);
    return c;
}

__global__ void __launch_bounds__(256) k_enc_count_ff(const ImgRec *__restrict__ imgs, int n, const uint64_t *__restrict__ img_bits,
                                                      const uint8_t *__restrict__ streams, uint32_t *__restrict__ chunk_ff)
{
    __shared__ unsigned waves[4];
    int img;
    uint64_t start, bytes;
    const uint2 v = chunk_bytes(imgs, n, blockIdx.x, img_bits, streams, img, start, bytes);
    const int lane = threadIdx.x & 63;
    const unsigned sum = wave_inclusive_sum(count_ff(v), lane);
    if (lane == 63) waves[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) chunk_ff[blockIdx.x] = waves[0] + waves[1] + waves[2] + waves[3];
}

__global__ void __launch_bounds__(256) k_enc_assemble(const ImgRec *__restrict__ imgs, int n, const uint64_t *__restrict__ img_bits,
                                                      const uint8_t *__restrict__ streams, const uint64_t *__restrict__ chunk_off,
                                                      const uint8_t *__restrict__ headers, const int64_t *__restrict__ offsets,
                                                      uint8_t *__restrict__ out, uint64_t capacity)
{
    __shared__ unsigned waves[4];
    int img;
    uint64_t start, bytes;
    const uint2 v = chunk_bytes(imgs, n, blockIdx.x, img_bits, streams, img, start, bytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned mine = count_ff(v);
    const unsigned sum = wave_inclusive_sum(mine, lane);
    if (lane == 63) waves[wave] = sum;
    __syncthreads();
    unsigned before = sum - mine;
    for (int i = 0; i < wave; ++i) before += waves[i];

    const unsigned hdr_len = imgs[img].hdr_len;
    const uint64_t file = (uint64_t)offsets[img];
    uint64_t at = file + hdr_len + start + chunk_off[blockIdx.x] + before;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (start + j >= bytes) break;
        const unsigned byte = ((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0xffu;
        if (at < capacity) out[at] = (uint8_t)byte;
        ++at;
        if (byte == 0xffu) {
            if (at < capacity) out[at] = 0;
            ++at;
        }
    }
    if (blockIdx.x != imgs[img].chunk0) return;
    // the image's first chunk: the header in front, EOI behind
    const uint8_t *hdr = headers + imgs[img].hdr_off;
    for (unsigned i = threadIdx.x; i < hdr_len; i += blockDim.x)
        if (file + i < capacity) out[file + i] = hdr[i];
    if (threadIdx.x < 2) {
        const uint64_t eoi = (uint64_t)offsets[img + 1] - 2 + threadIdx.x;
        if (eoi < capacity) out[eoi] = threadIdx.x ? 0xD9 : 0xFF;
    }
}

// ---- host: the Annex K tables, the headers ---------------------------------------------------------------------------------------

const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcValues[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The canonical codes of the four tables as the kernels index them: [luma, chroma][DC category 0 .. 15 | AC symbol 0 .. 255],
// (code << 8) | length.  Built by the first caller; the language makes every other thread wait (a function-local static).
struct HuffCodes {
    uint32_t e[2][kHuffStride];
    HuffCodes()
    {
        memset(e, 0, sizeof e);
        for (int t = 0; t < 2; t++) {
            uint32_t code = 0;
            int k = 0;
            for (int len = 1; len <= 16; len++, code <<= 1)
                for (int i = 0; i < kDcBits[t][len - 1]; i++) e[t][k++] = (code++ << 8) | (uint32_t)len;      // the DC symbols are 0 .. 11 in order
            code = 0;
            k = 0;
            for (int len = 1; len <= 16; len++, code <<= 1)
                for (int i = 0; i < kAcBits[t][len - 1]; i++) e[t][16 + kAcValues[t][k++]] = (code++ << 8) | (uint32_t)len;
        }
    }
};
const HuffCodes &huff_codes()
{
    static const HuffCodes codes;
    return codes;
}

void put_segment(std::vector<uint8_t> &out, int marker, const std::vector<uint8_t> &payload)
{
    const size_t len = payload.size() + 2;
    out.insert(out.end(), {0xFF, (uint8_t)marker, (uint8_t)(len >> 8), (uint8_t)len});
    out.insert(out.end(), payload.begin(), payload.end());
}

// SOI, APP0 (JFIF 1.1, no unit, 1 x 1), DQT per table, SOF0, DHT per table, SOS: what libjpeg writes before the scan
std::vector<uint8_t> build_header(int h, int w, int cn, const JpegTables &t)
{
    std::vector<uint8_t> out = {0xFF, 0xD8};
    put_segment(out, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    const int ntab = cn == 1 ? 1 : 2;
    for (int i = 0; i < ntab; i++) {
        std::vector<uint8_t> p = {(uint8_t)i};
        for (int z = 0; z < 64; z++) p.push_back((uint8_t)t.q[i][kZigzag[z]]);
        put_segment(out, 0xDB, p);
    }
    std::vector<uint8_t> sof = {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)cn};
    for (int c = 0; c < cn; c++) {
        sof.push_back((uint8_t)(c + 1));
        sof.push_back(cn == 3 && c == 0 ? 0x22 : 0x11);
        sof.push_back(c ? 1 : 0);
    }
    put_segment(out, 0xC0, sof);
    for (int i = 0; i < ntab; i++) {
        std::vector<uint8_t> dc = {(uint8_t)i};
        dc.insert(dc.end(), kDcBits[i], kDcBits[i] + 16);
        for (int v = 0; v < 12; v++) dc.push_back((uint8_t)v);
        put_segment(out, 0xC4, dc);
        std::vector<uint8_t> ac = {(uint8_t)(0x10 | i)};
        ac.insert(ac.end(), kAcBits[i], kAcBits[i] + 16);
        ac.insert(ac.end(), kAcValues[i], kAcValues[i] + 162);
        put_segment(out, 0xC4, ac);
    }
    std::vector<uint8_t> sos = {(uint8_t)cn};
    for (int c = 0; c < cn; c++) {
        sos.push_back((uint8_t)(c + 1));
        sos.push_back(c ? 0x11 : 0x00);
    }
    sos.insert(sos.end(), {0, 63, 0});
    put_segment(out, 0xDA, sos);
    return out;
}

}  // namespace

VKX_EXPORT int vkx_jpeg_encode_u8_dev(vkx_ctx *ctx, const vkx_jpeg_image *images_host, int n, int quality, int bgr, uint8_t *out,
                                      long long capacity, int64_t *offsets)
{
    VKX_REQUIRE(ctx && images_host && out && offsets, "NULL argument");
    VKX_REQUIRE(n >= 1 && n <= kMaxImages, "1 .. 65535 images");
    VKX_REQUIRE(0 <= quality && quality <= 100, "quality in 0 .. 100");
    VKX_REQUIRE(bgr == 0 || bgr == 1, "bgr is 0 or 1");
    VKX_REQUIRE(capacity >= 0, "negative capacity");
    VKX_REQUIRE((uintptr_t)offsets % 8 == 0, "offsets is not aligned to its element");

    // the records, and every source against the two destinations
    std::vector<ImgRec> recs((size_t)n);
    std::vector<std::pair<long long, long long>> dsts = {
        {(long long)(uintptr_t)offsets, (long long)((uintptr_t)offsets + 8 * ((size_t)n + 1))}};
    if (capacity) dsts.push_back({(long long)(uintptr_t)out, (long long)((uintptr_t)out + (size_t)capacity)});
    unsigned long long blocks = 0, groups = 0, chunks = 0;
    unsigned max_blocks = 0, max_chunks = 0;          // of one image: which shape its scans take
    for (int i = 0; i < n; i++) {
        const vkx_jpeg_image &im = images_host[i];
        VKX_REQUIRE(im.src != nullptr, "NULL source");
        VKX_REQUIRE(im.h >= 1 && im.h <= kMaxSide && im.w >= 1 && im.w <= kMaxSide, "a side outside 1 .. 32768");
        VKX_REQUIRE(im.cn == 1 || im.cn == 3, "1 or 3 channels");
        const long long s0 = (long long)(uintptr_t)im.src, s1 = s0 + (long long)im.h * im.w * im.cn;
        for (const auto &d : dsts) VKX_REQUIRE(s1 <= d.first || d.second <= s0, "a destination overlaps a source");
        ImgRec &r = recs[(size_t)i];
        r.src = im.src;
        r.h = im.h; r.w = im.w; r.cn = im.cn;
        r.ybw = (im.w + 7) / 8;
        r.ybh = (im.h + 7) / 8;
        r.mcus_x = (im.w + 15) / 16;
        const unsigned long long nblk = im.cn == 1 ? (unsigned long long)r.ybw * r.ybh
                                                   : 6ull * (unsigned long long)r.mcus_x * (unsigned long long)((im.h + 15) / 16);
        VKX_REQUIRE(blocks + nblk <= kMaxBlocks, "more than 2^26 blocks in one call");
        r.nblk = (unsigned)nblk;
        r.blk0 = (unsigned)blocks;
        r.wg0 = (unsigned)groups;
        r.chunk0 = (unsigned)chunks;
        r.nchunks = (unsigned)((nblk * kBlockBytes + kChunkBytes - 1) / kChunkBytes);
        blocks += nblk;
        max_blocks = std::max(max_blocks, r.nblk);
        max_chunks = std::max(max_chunks, r.nchunks);
        groups += (nblk + kBlocksPerGroup - 1) / kBlocksPerGroup;
        chunks += r.nchunks;
    }
    VKX_REQUIRE(dsts.size() < 2 || dsts[0].second <= dsts[1].first || dsts[1].second <= dsts[0].first, "out and offsets overlap");

    // one header per (channels, height, width)
    const JpegTables t = jpeg_tables(quality);
    std::map<std::tuple<int, int, int>, std::pair<unsigned, unsigned>> header_at;
    std::vector<uint8_t> headers;
    for (ImgRec &r : recs) {
        auto it = header_at.find({r.cn, r.h, r.w});
        if (it == header_at.end()) {
            const std::vector<uint8_t> hdr = build_header(r.h, r.w, r.cn, t);
            it = header_at.insert({{r.cn, r.h, r.w}, {(unsigned)headers.size(), (unsigned)hdr.size()}}).first;
            headers.insert(headers.end(), hdr.begin(), hdr.end());
        }
        r.hdr_off = it->second.first;
        r.hdr_len = it->second.second;
    }

    int rc;
    vkx_tables tab(ctx);
    const size_t rec_off = tab.add(sizeof(ImgRec) * (size_t)n), huff_off = tab.add(sizeof(HuffCodes)), hdr_off = tab.add(headers.size());
    if ((rc = tab.take())) return rc;
    memcpy(tab.at<ImgRec>(rec_off), recs.data(), sizeof(ImgRec) * (size_t)n);
    memcpy(tab.at<uint8_t>(huff_off), &huff_codes(), sizeof(HuffCodes));
    memcpy(tab.at<uint8_t>(hdr_off), headers.data(), headers.size());

    // the working set: coefficients, per-block bit counts and offsets, the unstuffed streams, per-chunk counts and offsets,
    // per-image bit counts and file sizes
    size_t bytes = 0;
    auto part = [&](size_t nbytes) { const size_t off = vkx_align256(bytes); bytes = off + nbytes; return off; };
    const size_t coef_off = part((size_t)blocks * 64 * sizeof(int16_t)), bits_off = part((size_t)blocks * 4);
    const size_t blk_off_off = part((size_t)blocks * 8), stream_off = part((size_t)blocks * kBlockBytes);
    const size_t ff_off = part((size_t)chunks * 4), chunk_off_off = part((size_t)chunks * 8);
    const size_t img_bits_off = part((size_t)n * 8), img_size_off = part((size_t)n * 8);
    if ((rc = vkx_scratch_reserve(ctx, &ctx->jpeg_encode_work, bytes))) return rc;
    if ((rc = tab.copy_to(&ctx->jpeg_encode_tables, (size_t)64 << 10))) return rc;      // grows (and syncs) rarely
    uint8_t *work = (uint8_t *)ctx->jpeg_encode_work.ptr;
    const uint8_t *tables = (const uint8_t *)ctx->jpeg_encode_tables.ptr;
    const ImgRec *imgs = (const ImgRec *)(tables + rec_off);
    const uint32_t *huff = (const uint32_t *)(tables + huff_off);
    int16_t *coef = (int16_t *)(work + coef_off);
    uint32_t *blk_bits = (uint32_t *)(work + bits_off), *chunk_ff = (uint32_t *)(work + ff_off);
    uint64_t *blk_off = (uint64_t *)(work + blk_off_off), *chunk_off = (uint64_t *)(work + chunk_off_off);
    uint64_t *img_bits = (uint64_t *)(work + img_bits_off), *img_size = (uint64_t *)(work + img_size_off);
    uint8_t *streams = work + stream_off;
    const unsigned total = (unsigned)blocks, waves4 = vkx_blocks(total, 4);
    {
        vkx_device_guard guard(ctx);
        VKX_HIP(hipMemsetAsync(streams, 0, (size_t)blocks * kBlockBytes, ctx->stream));
    }
    {
        VKX_TIMED(ctx, "k_enc_coef");
        k_enc_coef<<<(unsigned)groups, 256, 0, ctx->stream>>>(imgs, n, bgr, coef, t);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_lengths");
        k_enc_lengths<<<waves4, 256, 0, ctx->stream>>>(imgs, n, total, coef, huff, blk_bits);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_scan_blocks");
        if (max_blocks <= kScanSmallMax) k_enc_scan_blocks<ScanSmall><<<(unsigned)n, ScanSmall::kThreads, 0, ctx->stream>>>(imgs, blk_bits, blk_off, img_bits);
        else k_enc_scan_blocks<ScanLarge><<<(unsigned)n, ScanLarge::kThreads, 0, ctx->stream>>>(imgs, blk_bits, blk_off, img_bits);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_pack");
        k_enc_pack<<<waves4, 256, 0, ctx->stream>>>(imgs, n, total, coef, huff, blk_off, streams);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_count_ff");
        k_enc_count_ff<<<(unsigned)chunks, 256, 0, ctx->stream>>>(imgs, n, img_bits, streams, chunk_ff);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_scan_chunks");
        if (max_chunks <= kScanSmallMax) k_enc_scan_chunks<ScanSmall><<<(unsigned)n, ScanSmall::kThreads, 0, ctx->stream>>>(imgs, chunk_ff, img_bits, chunk_off, img_size);
        else k_enc_scan_chunks<ScanLarge><<<(unsigned)n, ScanLarge::kThreads, 0, ctx->stream>>>(imgs, chunk_ff, img_bits, chunk_off, img_size);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_offsets");
        if ((unsigned)n <= kScanSmallMax) k_enc_offsets<ScanSmall><<<1, ScanSmall::kThreads, 0, ctx->stream>>>(img_size, n, offsets);
        else k_enc_offsets<ScanLarge><<<1, ScanLarge::kThreads, 0, ctx->stream>>>(img_size, n, offsets);
        VKX_LAUNCH_CHECK();
    }
    {
        VKX_TIMED(ctx, "k_enc_assemble");
        k_enc_assemble<<<(unsigned)chunks, 256, 0, ctx->stream>>>(imgs, n, img_bits, streams, chunk_off, tables + hdr_off, offsets, out,
                                                                 (uint64_t)capacity);
        VKX_LAUNCH_CHECK();
    }
    return VKX_OK;
}
