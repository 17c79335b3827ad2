// Dropout of the Performer's dense sites (ff_dropout on the FF hidden h, attn_dropout on the attention output F; performer_pytorch 1.0.11 FeedForward /
// SelfAttention behind reference src/networks/transformers/performer.py:95-96,212-213).  Keep decisions: csrc/dropout.h, element index = flat index of the
// contiguous [rows, cols] tensor.  Every kernel walks groups of four consecutive elements, one Philox call per group.
#include "dropout.h"

namespace sa {

__device__ __forceinline__ int64_t drop_groups(int64_t n) { return (n + 3) >> 2; }

// out[e] = keep ? (scaled ? 1 / (1 - p) : 1) : 0
__global__ void dropout_mask_kernel(float* __restrict__ out, int64_t n, const DropParams d, int scaled) {
    const float one = scaled ? d.scale : 1.f;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < drop_groups(n); q += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 w = drop_words4(d, (uint64_t)q);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * q + r < n) out[4 * q + r] = w.v[r] >= d.thr ? one : 0.f;
    }
}

// x *= keep / (1 - p), in place (FF hidden h, the operand of w2)
template <typename T>
__global__ void dropout_apply_kernel(T* __restrict__ x, int64_t n, const DropParams d) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < drop_groups(n); q += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 w = drop_words4(d, (uint64_t)q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t e = 4 * q + r;
            if (e < n) DT<T>::st(x + e, w.v[r] >= d.thr ? DT<T>::ld(x + e) * d.scale : 0.f);
        }
    }
}

// du = dh * keep / (1 - p) * gelu'(u)   (the MASK_GELU data-gradient epilogue with the dropout mask in front)
template <typename TD, typename TU, typename TO>
__global__ void dropout_gelu_bwd_kernel(const TD* __restrict__ dh, const TU* __restrict__ u, TO* __restrict__ du, int64_t n, const DropParams d) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < drop_groups(n); q += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 w = drop_words4(d, (uint64_t)q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t e = 4 * q + r;
            if (e < n) DT<TO>::st(du + e, w.v[r] >= d.thr ? DT<TD>::ld(dh + e) * d.scale * gelu_grad_f(DT<TU>::ld(u + e)) : 0.f);
        }
    }
}

// F' = F * keep / (1 - p) (written back to F, kept for the gate gradient);  y = x + g F';  optional low-precision copy of y
template <typename TF>
__global__ void dropout_rezero_fwd_kernel(const float* __restrict__ x, TF* __restrict__ F, const float* __restrict__ g, float* __restrict__ y, void* y_lp,
                                          int lp_dtype, int64_t n, const DropParams d) {
    const float gv = g[0];
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < drop_groups(n); q += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 w = drop_words4(d, (uint64_t)q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t e = 4 * q + r;
            if (e >= n) continue;
            const float f = w.v[r] >= d.thr ? DT<TF>::ld(F + e) * d.scale : 0.f;
            DT<TF>::st(F + e, f);
            const float o = x[e] + gv * DT<TF>::ld(F + e);     // (the stored F', so the gate gradient <dy, F'> sees what the sum saw)
            y[e] = o;
            if (y_lp) store_from_f32(y_lp, lp_dtype, e, o);
        }
    }
}

// dF = g dy keep / (1 - p) ;  dg += sum dy F'   (F' = the dropped branch output of the forward)
template <typename TF, typename TO>
__global__ void dropout_rezero_bwd_kernel(const float* __restrict__ dy, const TF* __restrict__ F, const float* __restrict__ g, TO* __restrict__ dF,
                                          float* __restrict__ dg, int64_t n, const DropParams d) {
    const float gv = g[0];
    float s = 0.f;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < drop_groups(n); q += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 w = drop_words4(d, (uint64_t)q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t e = 4 * q + r;
            if (e >= n) continue;
            const float dv = dy[e];
            s += dv * DT<TF>::ld(F + e);
            DT<TO>::st(dF + e, w.v[r] >= d.thr ? gv * dv * d.scale : 0.f);
        }
    }
    s = wave_sum(s);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(dg, red[0] + red[1] + red[2] + red[3]);
}

static inline unsigned drop_grid(int64_t n) {
    const int64_t b = (((n + 3) >> 2) + 255) / 256;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, 8192));
}

static inline bool drop_args_ok(float p, int64_t n) { return n > 0 && p >= 0.f && p < 1.f; }

}  // namespace sa

using namespace sa;
#define ST(s) ((hipStream_t)(s))

extern "C" int sa_dropout_mask(float* out, int64_t n, float p, uint64_t seed, uint32_t site, int scaled, void* stream) {
    if (!out || !drop_args_ok(p, n)) return SA_EINVAL;
    SA_LAUNCH(dropout_mask_kernel, dim3(drop_grid(n)), dim3(256), 0, ST(stream), out, n, make_drop(p, seed, site), scaled);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_dropout_apply(void* x, int dtype, int64_t n, float p, uint64_t seed, uint32_t site, void* stream) {
    if (!x || !drop_args_ok(p, n)) return SA_EINVAL;
    const DropParams d = make_drop(p, seed, site);
    if (dtype == SA_F32) SA_LAUNCH(dropout_apply_kernel<float>, dim3(drop_grid(n)), dim3(256), 0, ST(stream), (float*)x, n, d);
    else if (dtype == SA_BF16) SA_LAUNCH(dropout_apply_kernel<bf16_t>, dim3(drop_grid(n)), dim3(256), 0, ST(stream), (bf16_t*)x, n, d);
    else return SA_EUNSUPPORTED;
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_dropout_gelu_bwd(const void* dh, int dh_dtype, const void* u, int u_dtype, void* du, int du_dtype, int64_t n, float p, uint64_t seed,
                                   uint32_t site, void* stream) {
    if (!dh || !u || !du || !drop_args_ok(p, n)) return SA_EINVAL;
    const DropParams d = make_drop(p, seed, site);
    const dim3 gr(drop_grid(n));
    if (dh_dtype == SA_F32 && u_dtype == SA_F32 && du_dtype == SA_F32)
        SA_LAUNCH((dropout_gelu_bwd_kernel<float, float, float>), gr, dim3(256), 0, ST(stream), (const float*)dh, (const float*)u, (float*)du, n, d);
    else if (dh_dtype == SA_BF16 && u_dtype == SA_BF16 && du_dtype == SA_BF16)
        SA_LAUNCH((dropout_gelu_bwd_kernel<bf16_t, bf16_t, bf16_t>), gr, dim3(256), 0, ST(stream), (const bf16_t*)dh, (const bf16_t*)u, (bf16_t*)du, n, d);
    else if (dh_dtype == SA_BF16 && u_dtype == SA_F32 && du_dtype == SA_BF16)
        SA_LAUNCH((dropout_gelu_bwd_kernel<bf16_t, float, bf16_t>), gr, dim3(256), 0, ST(stream), (const bf16_t*)dh, (const float*)u, (bf16_t*)du, n, d);
    else if (dh_dtype == SA_F32 && u_dtype == SA_F32 && du_dtype == SA_BF16)
        SA_LAUNCH((dropout_gelu_bwd_kernel<float, float, bf16_t>), gr, dim3(256), 0, ST(stream), (const float*)dh, (const float*)u, (bf16_t*)du, n, d);
    else return SA_EUNSUPPORTED;
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_dropout_rezero_fwd(const float* x, void* F, int f_dtype, const float* g, float* y, void* y_lp, int lp_dtype, int64_t n, float p, uint64_t seed,
                                     uint32_t site, void* stream) {
    if (!x || !F || !g || !y || !drop_args_ok(p, n)) return SA_EINVAL;
    const DropParams d = make_drop(p, seed, site);
    if (f_dtype == SA_F32)
        SA_LAUNCH(dropout_rezero_fwd_kernel<float>, dim3(drop_grid(n)), dim3(256), 0, ST(stream), x, (float*)F, g, y, y_lp, lp_dtype, n, d);
    else if (f_dtype == SA_BF16)
        SA_LAUNCH(dropout_rezero_fwd_kernel<bf16_t>, dim3(drop_grid(n)), dim3(256), 0, ST(stream), x, (bf16_t*)F, g, y, y_lp, lp_dtype, n, d);
    else return SA_EUNSUPPORTED;
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_dropout_rezero_bwd(const float* dy, const void* F, int f_dtype, const float* g, void* dF, int df_dtype, float* dg, int64_t n, float p,
                                     uint64_t seed, uint32_t site, void* stream) {
    if (!dy || !F || !g || !dF || !dg || !drop_args_ok(p, n)) return SA_EINVAL;
    const DropParams d = make_drop(p, seed, site);
    const dim3 gr(drop_grid(n));
    if (f_dtype == SA_F32 && df_dtype == SA_F32)
        SA_LAUNCH((dropout_rezero_bwd_kernel<float, float>), gr, dim3(256), 0, ST(stream), dy, (const float*)F, g, (float*)dF, dg, n, d);
    else if (f_dtype == SA_F32 && df_dtype == SA_BF16)
        SA_LAUNCH((dropout_rezero_bwd_kernel<float, bf16_t>), gr, dim3(256), 0, ST(stream), dy, (const float*)F, g, (bf16_t*)dF, dg, n, d);
    else if (f_dtype == SA_BF16 && df_dtype == SA_BF16)
        SA_LAUNCH((dropout_rezero_bwd_kernel<bf16_t, bf16_t>), gr, dim3(256), 0, ST(stream), dy, (const bf16_t*)F, g, (bf16_t*)dF, dg, n, d);
    else return SA_EUNSUPPORTED;
    SA_CHECK_LAUNCH();
    return 0;
}
