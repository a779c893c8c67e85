// cv.warpAffine's coordinate generator (imgwarp.cpp, AB_BITS = 10 fixed point), shared by the warp kernels of remap.hip and
// the batched region warp of region_flatten.hip: one statement of the arithmetic, bit for bit oracle/vkx_oracle.c's.
#pragma once
#include "vkx_internal.h"

namespace vkd {

struct CoordAffine {   // warpAffine: inverse matrix, AB_BITS = 10 fixed point
    // a rotated / sheared source footprint: 64 destination pixels of ONE row reach a slanted strip of the source (6 degrees:
    // 8 source rows, ~32 cache lines per tap-load instruction); a wavefront therefore takes 16 columns x 4 rows per instruction
    // (5 - 6 lines), four wavefronts side by side so that their 48-byte row segments complete cache lines on the way out
    static constexpr bool kTile2D = true;
    double m[6];
    // adelta[x] / bdelta[x] of cv::warpAffine depend on the column only: a lane that walks several rows of its column
    // computes them once
    struct Column { int adelta, bdelta; };
    __device__ __forceinline__ Column column(int x) const
    {
        return Column{vkd::cv_round(m[0] * x * 1024), vkd::cv_round(m[3] * x * 1024)};
    }
    // X0 / Y0 of cv::warpAffine depend on the row only: lane r of the wavefront computes those of row y0 + r (one double
    // evaluation per wavefront instead of one per row), every lane reads them back with v_readlane
    struct Rows { int X0, Y0; };
    __device__ __forceinline__ Rows rows(int y0, int lane) const
    {
        const int y = y0 + (lane & 15);
        return Rows{vkd::cv_round((m[1] * y + m[2]) * 1024) + 16, vkd::cv_round((m[4] * y + m[5]) * 1024) + 16};
    }
    // `row`: the lane's row inside the tile (0 .. 15), per lane: the row terms come from the lane that computed them
    __device__ __forceinline__ void at(const Column &c, const Rows &r, int row, int, int, int &X, int &Y) const
    {
        X = (__builtin_amdgcn_ds_bpermute(row << 2, r.X0) + c.adelta) >> 5;
        Y = (__builtin_amdgcn_ds_bpermute(row << 2, r.Y0) + c.bdelta) >> 5;
    }
    __device__ __forceinline__ void operator()(int x, int y, int &X, int &Y) const
    {
        const int adelta = vkd::cv_round(m[0] * x * 1024);
        const int bdelta = vkd::cv_round(m[3] * x * 1024);
        const int X0 = vkd::cv_round((m[1] * y + m[2]) * 1024) + 16;
        const int Y0 = vkd::cv_round((m[4] * y + m[5]) * 1024) + 16;
        X = (X0 + adelta) >> 5;
        Y = (Y0 + bdelta) >> 5;
    }
};

// cv::warpAffine's in-place inversion of the forward 2x3 matrix (double).
inline CoordAffine make_affine(const double Mf[6])
{
    CoordAffine c;
    double M[6];
    for (int i = 0; i < 6; i++) M[i] = Mf[i];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int i = 0; i < 6; i++) c.m[i] = M[i];
    return c;
}

} // namespace vkd
