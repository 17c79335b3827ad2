// What the HBM-bound FAVOR+ projection kernels share (favor_proj.hip: the softmax random-feature map; favor_generalized.hip: the ReLU map):
// addressing of head blocks inside wider rows, staging of the projection matrix in LDS as split-bf16 hi / lo tiles, and the bit mask that
// zeroes the operands of rows past the end.
#pragma once
#include "sa_common.h"
#include "split_bf16.h"

namespace sa {

__device__ __forceinline__ int64_t proj_row_off(int64_t r, int heads, int stride) { return (r / heads) * stride + (r % heads) * 64; }

// projection rows [0, nrows) -> hi / lo tiles [nrows][64] bf16 in the lroff() layout (rows >= m are zero)
// PERM: tile row rho holds projection row pi(rho), pi(ks*32 + b*16 + 4g + r) = ks*32 + 8g + 4b + r.  The transposing reads hand lane group g the
// tile rows {4g..4g+3, 16+4g..} of a 32-row block as its eight reduction steps; with pi those are the EIGHT CONSECUTIVE features ks*32 + 8g .. +7,
// so the gradient rows that multiply them are read as 32 contiguous bytes per lane (a full 128-byte line per row and 32-feature block).
template <bool PERM = false>
__device__ __forceinline__ void proj_stage(unsigned char* hi, unsigned char* lo, const float* proj, int m, int nrows, int tid) {
    // all loads first (nrows <= 288: at most 18 pieces of 16 bytes per thread), then the splits: a load -> split -> store loop with a run-time
    // trip count pays the L2 round trip once per iteration (18 us per block, measured as 2/3 of the adjoint kernel)
    float4 v[18];
#pragma unroll
    for (int t = 0; t < 18; ++t) {
        const int idx = tid + 256 * t, rho = min(idx >> 4, nrows - 1), c4 = idx & 15;
        const int f = PERM ? (rho & ~31) | (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3) : rho;
        v[t] = *(const float4*)(proj + (int64_t)min(f, m - 1) * 64 + c4 * 4);
    }
#pragma unroll
    for (int t = 0; t < 18; ++t) {
        const int idx = tid + 256 * t, rho = idx >> 4, c4 = idx & 15;
        if (rho < nrows) {
            const int f = PERM ? (rho & ~31) | (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3) : rho;
            const float k = f < m ? 1.f : 0.f;
            uint2 h, l;
            split_pair(v[t].x * k, v[t].y * k, h.x, l.x);
            split_pair(v[t].z * k, v[t].w * k, h.y, l.y);
            const uint32_t o = lroff(rho, c4 * 4);
            *(uint2*)(hi + o) = h;
            *(uint2*)(lo + o) = l;
        }
    }
}

__device__ __forceinline__ float4 proj_keep(float4 x, bool keep) {
    const uint32_t mk = keep ? 0xffffffffu : 0u;
    return make_float4(__uint_as_float(__float_as_uint(x.x) & mk), __uint_as_float(__float_as_uint(x.y) & mk), __uint_as_float(__float_as_uint(x.z) & mk),
                       __uint_as_float(__float_as_uint(x.w) & mk));
}

}  // namespace sa
