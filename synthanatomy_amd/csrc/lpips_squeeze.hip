// The two ends of the LPIPS-squeeze chain (BaselineLoss of the reference, src/losses/vqvae/vqvae.py:1648-1780, and lpips_kwargs net="squeeze"; DESIGN.md
// section 7.13): the first layer of SqueezeNet-1.1 and its adjoint.  The Fire modules run on the MFMA implicit-GEMM sa_conv_fprop, the seven taps go through
// sa_lpips_head, and the ceil-mode pools (sa_lpips_maxpool_ceil_fwd / _bwd) share their kernels with the floor-mode pair in csrc/lpips.hip; the slice view
// and the extent guard are in csrc/lpips_common.h.
//   sa_lpips_squeeze_conv1_fwd : Conv(3 -> 64, k3, s2, p0) + ReLU of the scaled, channel-broadcast slice, read straight from the fp32 volume by (view, slice
//                                id) like sa_lpips_unfold, written channels-last [S, h1, w1, 64].  The scaling layer is folded into the caller's [9][64]
//                                weights and bias; with no padding the fold is exact everywhere (no border classes).  Cin = 1 x 9 taps is a bandwidth kernel:
//                                a slice is read once (L2 serves the overlapping windows), 64 channels are written per position.
//   sa_lpips_squeeze_conv1_bwd : its adjoint: one thread per voxel of the kept slices sums the <= 2 x 2 covering positions x 64 channels in a fixed order,
//                                applies the tap's ReLU mask, scales and ACCUMULATES into the fp32 volume gradient (no atomics: the ids are distinct)
#include "lpips_common.h"

namespace sa {

constexpr int SQ_K = 3, SQ_S = 2, SQ_TAPS = 9, SQ_C = 64;

static inline int sq_conv1_out(int e) { return (e - SQ_K) / SQ_S + 1; }

struct SqConv1 {
    const float* x;         // forward: the fp32 volume
    const float* w;         // [9][64] fp32, tap-major, scaling layer folded in
    const float* bias;      // [64]
    void* y;                // forward: [S, ho, wo, 64] T
    const void* gy;         // backward: [S, ho, wo, 64] T, gradient at the tap (post-ReLU)
    const void* mask;       // backward: [S, ho, wo, 64] T or NULL: the tap itself; gy counts where mask > 0
    float* grad;            // backward: [B, D, H, W] fp32, accumulated
    const int32_t* ids;
    LpView v;
    int32_t S, B, ho, wo, normalize;
    float scale;
    uint32_t total;
    FastDiv dA, dB;         // forward: wo, ho; backward: w, h
};

// thread = (output position, 8 consecutive channels): 9 broadcast reads of the slice, one 16-byte (bf16) or two 16-byte (fp32) stores
template <typename T>
__global__ __launch_bounds__(256) void squeeze_conv1_fwd_kernel(const SqConv1 a) {
    __shared__ float sw[SQ_TAPS * SQ_C], sb[SQ_C];
    for (int i = threadIdx.x; i < SQ_TAPS * SQ_C; i += 256) sw[i] = a.w[i];
    if (threadIdx.x < SQ_C) sb[threadIdx.x] = a.bias[threadIdx.x];
    __syncthreads();
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.total) return;
    const int c0 = (int)(e & 7u) * 8;
    const uint32_t pos = e >> 3;
    uint32_t q = fdiv(pos, a.dA);
    const int ow = (int)(pos - q * (uint32_t)a.wo);
    const uint32_t s = fdiv(q, a.dB);
    const int oh = (int)(q - s * (uint32_t)a.ho);
    const int sid = a.ids[s];
    const bool live = (unsigned)sid < (unsigned)(a.B * a.v.n);       // (an id outside the view reads nothing: its taps are zero)
    const int b = live ? sid / a.v.n : 0, ax = live ? sid - b * a.v.n : 0;
    // (2 oh + 2 <= h - 1 by the floor extent: every window lies inside the slice)
    const float* sl = a.x + (int64_t)b * a.v.sb + (int64_t)ax * a.v.sa + (int64_t)(oh * SQ_S) * a.v.si + (int64_t)(ow * SQ_S) * a.v.sj;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = sb[c0 + c];
#pragma unroll
    for (int t = 0; t < SQ_TAPS; ++t) {
        float xv = 0.f;
        if (live) {
            xv = sl[(int64_t)(t / SQ_K) * a.v.si + (int64_t)(t % SQ_K) * a.v.sj];
            if (a.normalize) xv = 2.f * xv - 1.f;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] += xv * sw[t * SQ_C + c0 + c];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = fmaxf(acc[c], 0.f);
    unsigned char* dst = (unsigned char*)a.y + ((size_t)pos * SQ_C + c0) * sizeof(T);
    if constexpr (sizeof(T) == 4) {
        *(float4*)dst = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *(float4*)(dst + 16) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
        uint4 pk;
        pk.x = pack2<T>(acc[0], acc[1]);
        pk.y = pack2<T>(acc[2], acc[3]);
        pk.z = pack2<T>(acc[4], acc[5]);
        pk.w = pack2<T>(acc[6], acc[7]);
        *(uint4*)dst = pk;
    }
}

// thread = one voxel of a kept slice; covering positions in the order oh, ow, channels in order: one fixed sum per voxel
template <typename T>
__global__ __launch_bounds__(256) void squeeze_conv1_bwd_kernel(const SqConv1 a) {
    __shared__ float sw[SQ_TAPS * SQ_C];
    for (int i = threadIdx.x; i < SQ_TAPS * SQ_C; i += 256) sw[i] = a.w[i];
    __syncthreads();
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.total) return;
    uint32_t q = fdiv(idx, a.dA);
    const int j = (int)(idx - q * (uint32_t)a.v.w);
    const uint32_t s = fdiv(q, a.dB);
    const int i = (int)(q - s * (uint32_t)a.v.h);
    const int sid = a.ids[s];
    if ((unsigned)sid >= (unsigned)(a.B * a.v.n)) return;
    // oh covers i when 0 <= i - 2 oh < 3
    const int oh_lo = max((i - 1) / 2, 0), oh_hi = min(i / 2, a.ho - 1), ow_lo = max((j - 1) / 2, 0), ow_hi = min(j / 2, a.wo - 1);
    float sum = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        const int ti = i - SQ_S * oh;
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            const int tj = j - SQ_S * ow;
            const int64_t o = (((int64_t)s * a.ho + oh) * a.wo + ow) * SQ_C;
            const float* wt = sw + (ti * SQ_K + tj) * SQ_C;
#pragma unroll 8
            for (int c = 0; c < SQ_C; ++c) {
                float g = DT<T>::ld((const T*)a.gy + o + c);
                if (a.mask && !(DT<T>::ld((const T*)a.mask + o + c) > 0.f)) g = 0.f;
                sum += g * wt[c];
            }
        }
    }
    const int b = sid / a.v.n, ax = sid - b * a.v.n;
    float* g = a.grad + (int64_t)b * a.v.sb + (int64_t)ax * a.v.sa + (int64_t)i * a.v.si + (int64_t)j * a.v.sj;
    *g += a.scale * sum;
}

static int sq_conv1_args(SqConv1& a, int dtype, int S, int view, int B, int D, int H, int W, bool bwd) {
    if (S <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0 || !make_view(view, D, H, W, a.v)) return SA_EINVAL;
    if (dtype != SA_F32 && dtype != SA_BF16) return SA_EUNSUPPORTED;
    if (a.v.h < SQ_K || a.v.w < SQ_K) return SA_EINVAL;
    a.ho = sq_conv1_out(a.v.h); a.wo = sq_conv1_out(a.v.w);
    const int64_t pos = (int64_t)S * a.ho * a.wo, vox = (int64_t)S * a.v.h * a.v.w;
    if (!lp_ok(pos * 8) || !lp_ok(vox) || !lp_ok((int64_t)B * D * H * W) || !lp_ok((int64_t)B * a.v.n)) return SA_EINVAL;
    a.S = S; a.B = B;
    a.total = (uint32_t)(bwd ? vox : pos * 8);
    a.dA = make_fastdiv((uint32_t)(bwd ? a.v.w : a.wo)); a.dB = make_fastdiv((uint32_t)(bwd ? a.v.h : a.ho));
    return 0;
}

}  // namespace sa

extern "C" int sa_lpips_squeeze_conv1_fwd(const float* x, int dtype, const float* w, const float* bias, void* y, const int32_t* slice_ids, int S, int view, int B,
                                          int D, int H, int W, int normalize, void* stream) {
    using namespace sa;
    if (!x || !w || !bias || !y || !slice_ids) return SA_EINVAL;
    SqConv1 a = {};
    const int rc = sq_conv1_args(a, dtype, S, view, B, D, H, W, false);
    if (rc) return rc;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.ids = slice_ids; a.normalize = normalize;
    const dim3 grid((a.total + 255u) / 256u);
    LP_LAUNCH_T(dtype, squeeze_conv1_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_lpips_squeeze_conv1_bwd(const void* gy, const void* mask, int dtype, const float* w, float* grad, const int32_t* slice_ids, int S, int view,
                                          int B, int D, int H, int W, float scale, void* stream) {
    using namespace sa;
    if (!gy || !w || !grad || !slice_ids) return SA_EINVAL;
    SqConv1 a = {};
    const int rc = sq_conv1_args(a, dtype, S, view, B, D, H, W, true);
    if (rc) return rc;
    a.gy = gy; a.mask = mask; a.w = w; a.grad = grad; a.ids = slice_ids; a.scale = scale;
    const dim3 grid((a.total + 255u) / 256u);
    LP_LAUNCH_T(dtype, squeeze_conv1_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}
