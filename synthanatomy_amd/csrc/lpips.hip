// The memory-bound kernels of the 2.5D LPIPS-alex perceptual term (PerceptualLoss / JukeboxPerceptualLoss / HartleyPerceptualLoss of the reference,
// src/losses/vqvae/vqvae.py:774-1645).  The five convolutions run on the MFMA implicit-GEMM sa_conv_fprop; these kernels move the
// data between them:
//   sa_lpips_unfold       : kept slices of one 2.5D view, read straight from the fp32 volume [B, 1, D, H, W] (no permuted copy exists), -> the operand
//                           of conv1 as a 1-tap GEMM: the 11 x 11 / stride 4 / pad 2 taps of u = 2x - 1 as columns, ZERO outside the image
//   sa_lpips_fold         : the inverse for the data gradient: one thread per voxel of the view's kept slices gathers the <= 3 x 3 output positions that
//                           cover it in a fixed order and accumulates into the volume gradient (no atomics: the slices of a view are distinct)
//   sa_lpips_maxpool_fwd  : MaxPool2d(3, 2), channels-last, floor extents, first maximum in row-major window order (torch's tie rule), + its argmax
//   sa_lpips_maxpool_bwd  : the gather form of its gradient, fused with the addend (the LPIPS head's own gradient at that tap) and the ReLU mask
//   sa_lpips_maxpool_ceil_fwd / _bwd : the same pair with MaxPool2d(3, 2, ceil_mode=True) extents for the LPIPS-squeeze chain:
//                           the last window may overhang and is clipped to the map.  One kernel pair serves both extent rules
//   sa_lpips_head         : per tap: unit-normalise both feature maps over channels, d[s] += mean_hw sum_c w_c (f0^ - f1^)^2 and, in the same pass,
//                           d d / d f1 (the loss-and-gradient-in-one-pass pattern of sa_baur_loss)
// The slice view and the extent guard are in csrc/lpips_common.h, shared with csrc/lpips_squeeze.hip.
//
// THE PADDING RULE.  Upstream scales the image, (u - shift_c) / scale_c, and conv1 then zero-pads the SCALED image: a padded tap contributes 0, not
// -shift_c / scale_c.  Folding shift and scale into conv1's weights and bias is therefore exact only where the window lies inside the image.  The
// unfold kernel keeps the fold exact at the border without a second pass: besides the 121 taps, a row carries a one-hot of its BORDER CLASS
// (interior / top / bottom) x (interior / left / right) in columns 121 .. 129, and the caller's weight matrix holds, in those nine columns,
// -sum over the taps that are INSIDE the image for that class of sum_c W[o, c, t] shift_c / scale_c.  A constant image shows the difference.
//
// THE SUBGRADIENT AT ZERO.  f^ = f / (sqrt(sum_c f^2) + 1e-10).  Where the feature vector of the prediction is all zero, autograd's gradient of
// the square root is NaN (0 / 0); this kernel takes the subgradient 0 there, i.e. it drops the projection term and writes q / 1e-10, which the ReLU mask
// of the layer (every f is 0 there) then turns into an exact 0.  A deliberate difference from upstream: the gradient is finite everywhere.
#include "lpips_common.h"

namespace sa {

constexpr int LP_K = 11, LP_S = 4, LP_P = 2, LP_TAPS = LP_K * LP_K, LP_CLS = 9;

static inline int conv1_out(int e) { return (e + 2 * LP_P - LP_K) / LP_S + 1; }
__device__ __forceinline__ int border_class(int o, int e) { return o * LP_S - LP_P < 0 ? 1 : (o * LP_S - LP_P + LP_K - 1 >= e ? 2 : 0); }

struct LpUnfold {
    const float* x;
    void* cols;             // [S, ho, wo, ld] T
    const int32_t* ids;     // [S] slice ids of the view
    LpView v;
    int32_t S, B, ho, wo, ld, normalize;
    uint32_t rows, chunks, rpb;
    FastDiv dWo, dHo, dCh;
};

// thread = (row, 16-byte chunk of its row), as taps_unfold_kernel: a block writes `rpb` consecutive rows, 16 bytes per lane
template <typename T>
__global__ __launch_bounds__(256) void lpips_unfold_kernel(const LpUnfold a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const uint32_t tid = threadIdx.x;
    const uint32_t lr = fdiv(tid, a.dCh), ch = tid - lr * a.chunks;
    if (lr >= a.rpb) return;
    for (uint32_t row = blockIdx.x * a.rpb + lr; row < a.rows; row += gridDim.x * a.rpb) {
        uint32_t q = fdiv(row, a.dWo);
        const int ow = (int)(row - q * (uint32_t)a.wo);
        const uint32_t s = fdiv(q, a.dHo);
        const int oh = (int)(q - s * (uint32_t)a.ho);
        const int sid = a.ids[s];
        const bool live = (unsigned)sid < (unsigned)(a.B * a.v.n);       // (an id outside the view reads nothing: its row is zero)
        const int b = sid / a.v.n, ax = sid - b * a.v.n;
        const float* sl = a.x + (int64_t)b * a.v.sb + (int64_t)ax * a.v.sa;
        const int bi = oh * LP_S - LP_P, bj = ow * LP_S - LP_P;
        const int cls = border_class(oh, a.v.h) * 3 + border_class(ow, a.v.w);
        float val[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int t = (int)ch * VEC + e;
            const int ti = t / LP_K, tj = t - ti * LP_K;
            const int i = bi + ti, j = bj + tj;
            float r = 0.f;
            if (t < LP_TAPS) {
                if (live && (unsigned)i < (unsigned)a.v.h && (unsigned)j < (unsigned)a.v.w) {
                    const float xv = sl[(int64_t)i * a.v.si + (int64_t)j * a.v.sj];
                    r = a.normalize ? 2.f * xv - 1.f : xv;
                }
            } else if (t < LP_TAPS + LP_CLS) {
                r = live && (t - LP_TAPS) == cls ? 1.f : 0.f;
            }
            val[e] = r;
        }
        unsigned char* dst = (unsigned char*)a.cols + ((size_t)row * a.ld) * sizeof(T) + (size_t)ch * 16;
        if constexpr (sizeof(T) == 4) {
            *(float4*)dst = make_float4(val[0], val[1], val[2], val[3]);
        } else {
            uint4 pk;
            pk.x = pack2<T>(val[0], val[1]);
            pk.y = pack2<T>(val[2], val[3]);
            pk.z = pack2<T>(val[4], val[5]);
            pk.w = pack2<T>(val[6], val[7]);
            *(uint4*)dst = pk;
        }
    }
}

struct LpFold {
    const float* dcols;     // [S, ho, wo, ld] fp32: d / d (columns)
    float* grad;            // [B, D, H, W] fp32, accumulated
    const int32_t* ids;
    LpView v;
    int32_t S, B, ho, wo, ld;
    float scale;
    uint32_t total;         // S * h * w
    FastDiv dW, dH;
};

// thread = one voxel of a kept slice; output positions in the order oh, ow: one fixed sum per voxel
__global__ __launch_bounds__(256) void lpips_fold_kernel(const LpFold a) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.total) return;
    uint32_t q = fdiv(idx, a.dW);
    const int j = (int)(idx - q * (uint32_t)a.v.w);
    const uint32_t s = fdiv(q, a.dH);
    const int i = (int)(q - s * (uint32_t)a.v.h);
    const int sid = a.ids[s];
    if ((unsigned)sid >= (unsigned)(a.B * a.v.n)) return;
    // oh covers i when 0 <= i + P - oh * S < K
    const int oh_hi = min((i + LP_P) / LP_S, a.ho - 1), ow_hi = min((j + LP_P) / LP_S, a.wo - 1);
    const int oh_lo = max((i + LP_P - LP_K + LP_S) / LP_S, 0), ow_lo = max((j + LP_P - LP_K + LP_S) / LP_S, 0);
    float sum = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        const int ti = i + LP_P - oh * LP_S;
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            const int tj = j + LP_P - ow * LP_S;
            sum += a.dcols[(((int64_t)s * a.ho + oh) * a.wo + ow) * a.ld + ti * LP_K + tj];
        }
    }
    const int b = sid / a.v.n, ax = sid - b * a.v.n;
    float* g = a.grad + (int64_t)b * a.v.sb + (int64_t)ax * a.v.sa + (int64_t)i * a.v.si + (int64_t)j * a.v.sj;
    *g += a.scale * sum;
}

struct LpPool {
    const void* x;          // [S, Hi, Wi, C]
    void* y;                // [S, Ho, Wo, C]
    unsigned char* idx;     // [S, Ho, Wo, C]: position 3 * kh + kw of the maximum, counted in the FULL (unclipped) window under both extent rules
    const void* gy;         // backward: [S, Ho, Wo, C]
    const void* addend;     // backward: [S, Hi, Wi, C] or NULL
    const void* mask;       // backward: [S, Hi, Wi, C] or NULL: gx *= (mask > 0)
    void* gx;               // backward: [S, Hi, Wi, C]
    int32_t Hi, Wi, Ho, Wo, C;
    uint64_t total;
};

// thread = one (output position, channel); lanes run along the channels (coalesced).  CLIP = false: floor extents, 2 * oh + 2 < Hi, every window lies
// inside the map.  CLIP = true: ceil extents, the last window may overhang and is clipped to the map (it STARTS inside: the extent drops one that would not).
template <typename T, bool CLIP>
__global__ __launch_bounds__(256) void lpips_maxpool_fwd_kernel(const LpPool a) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= a.total) return;
    const int c = (int)(e % (uint32_t)a.C);
    uint64_t p = e / (uint32_t)a.C;
    const int ow = (int)(p % (uint32_t)a.Wo); p /= (uint32_t)a.Wo;
    const int oh = (int)(p % (uint32_t)a.Ho);
    const int64_t s = (int64_t)(p / (uint32_t)a.Ho);
    const int ih = 2 * oh, iw = 2 * ow;
    const T* x = (const T*)a.x + ((s * a.Hi + ih) * a.Wi + iw) * a.C + c;
    float best = DT<T>::ld(x);
    int arg = 0;
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        if (!CLIP || (ih + k / 3 < a.Hi && iw + k % 3 < a.Wi)) {
            const float v = DT<T>::ld(x + ((int64_t)(k / 3) * a.Wi + (k % 3)) * a.C);
            if (v > best || v != v) { best = v; arg = k; }      // strictly greater: the FIRST maximum wins (NaN propagates, as in torch)
        }
    }
    DT<T>::st((T*)a.y + e, best);
    a.idx[e] = (unsigned char)arg;
}

// thread = one (input position, channel): the <= 2 x 2 windows that contain it, in the order oh, ow (the range is clamped by Ho / Wo, so it serves both
// extent rules).  Floor extents: a trailing row / column no window covers gets 0 (+ addend).  Ceil extents: every position is covered.
template <typename T>
__global__ __launch_bounds__(256) void lpips_maxpool_bwd_kernel(const LpPool a) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= a.total) return;
    const int c = (int)(e % (uint32_t)a.C);
    uint64_t p = e / (uint32_t)a.C;
    const int iw = (int)(p % (uint32_t)a.Wi); p /= (uint32_t)a.Wi;
    const int ih = (int)(p % (uint32_t)a.Hi);
    const int64_t s = (int64_t)(p / (uint32_t)a.Hi);
    float sum = a.addend ? DT<T>::ld((const T*)a.addend + e) : 0.f;
    const int oh_lo = max((ih - 1) / 2, 0), oh_hi = min(ih / 2, a.Ho - 1), ow_lo = max((iw - 1) / 2, 0), ow_hi = min(iw / 2, a.Wo - 1);
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            const int64_t o = ((s * a.Ho + oh) * a.Wo + ow) * a.C + c;
            if ((int)a.idx[o] == (ih - 2 * oh) * 3 + (iw - 2 * ow)) sum += DT<T>::ld((const T*)a.gy + o);
        }
    if (a.mask && !(DT<T>::ld((const T*)a.mask + e) > 0.f)) sum = 0.f;
    DT<T>::st((T*)a.gx + e, sum);
}

struct LpHead {
    const void *f0, *f1;    // [S, P, C]
    const float* w;         // [C] lin weights
    float* d;               // [S], accumulated
    void* g1;               // [S, P, C] or NULL
    int32_t P, C, relu_mask;
    float inv_p;
};

constexpr int LP_MAXC = 512;    // channels per position: <= 8 per lane

// block = one slice, wave = every fourth position, lane = channels lane, lane + 64, ...: both feature vectors are read once and stay in registers for
// the gradient.  Reductions: butterfly over the wave, positions in order per wave, the four waves in order -- one fixed order, bitwise repeatable.
template <typename T>
__global__ __launch_bounds__(256) void lpips_head_kernel(const LpHead a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t s = blockIdx.x;
    const int nj = (a.C + 63) / 64;
    float wl[LP_MAXC / 64];
#pragma unroll
    for (int j = 0; j < LP_MAXC / 64; ++j) wl[j] = (j < nj && lane + 64 * j < a.C) ? a.w[lane + 64 * j] : 0.f;
    float dsum = 0.f;
    for (int p = wv; p < a.P; p += 4) {
        const int64_t base = (s * a.P + p) * a.C;
        float x0[LP_MAXC / 64], x1[LP_MAXC / 64];
        float n0 = 0.f, n1 = 0.f;
#pragma unroll
        for (int j = 0; j < LP_MAXC / 64; ++j) {
            const bool ok = j < nj && lane + 64 * j < a.C;
            x0[j] = ok ? DT<T>::ld((const T*)a.f0 + base + lane + 64 * j) : 0.f;
            x1[j] = ok ? DT<T>::ld((const T*)a.f1 + base + lane + 64 * j) : 0.f;
            n0 += x0[j] * x0[j];
            n1 += x1[j] * x1[j];
        }
        n0 = wave_sum(n0);
        n1 = wave_sum(n1);
        const float r1 = sqrtf(n1);
        const float i0 = 1.f / (sqrtf(n0) + 1e-10f), i1 = 1.f / (r1 + 1e-10f);
        float dp = 0.f, dot = 0.f;
        float qv[LP_MAXC / 64];
#pragma unroll
        for (int j = 0; j < LP_MAXC / 64; ++j) {
            const float df = x1[j] * i1 - x0[j] * i0;
            dp += wl[j] * df * df;
            qv[j] = 2.f * wl[j] * df * a.inv_p;
            dot += qv[j] * x1[j];
        }
        dsum += wave_sum(dp);
        if (a.g1) {
            dot = wave_sum(dot);
            // d f^_c / d f_k = delta_ck / (r + eps) - f_c f_k / ((r + eps)^2 r); at r = 0 the projection term is dropped (subgradient 0 of the square root)
            const float proj = r1 > 0.f ? dot * i1 * i1 / r1 : 0.f;
#pragma unroll
            for (int j = 0; j < LP_MAXC / 64; ++j) {
                if (j < nj && lane + 64 * j < a.C) {
                    float g = qv[j] * i1 - x1[j] * proj;
                    if (a.relu_mask && !(x1[j] > 0.f)) g = 0.f;
                    DT<T>::st((T*)a.g1 + base + lane + 64 * j, g);
                }
            }
        }
    }
    __shared__ float red[4];
    if (lane == 0) red[wv] = dsum;
    __syncthreads();
    if (threadIdx.x == 0) a.d[s] += (((red[0] + red[1]) + red[2]) + red[3]) * a.inv_p;
}

static inline int ceil_pool_out(int e) {
    int o = (e - 3 + 1) / 2 + 1;        // ceil((e - 3) / 2) + 1 for e >= 2
    if ((o - 1) * 2 >= e) --o;          // the last window would start outside the map
    return o;
}

// floor extents (e - 3) / 2 + 1, sides >= 3; ceil extents as MaxPool2d(ceil_mode=True), sides >= 2
static int pool_args(LpPool& a, int dtype, int S, int Hi, int Wi, int C, bool ceil, bool bwd) {
    if (dtype != SA_F32 && dtype != SA_BF16) return SA_EUNSUPPORTED;
    const int side = ceil ? 2 : 3;
    if (S <= 0 || Hi < side || Wi < side || C <= 0) return SA_EINVAL;
    a.Hi = Hi; a.Wi = Wi; a.C = C;
    a.Ho = ceil ? ceil_pool_out(Hi) : (Hi - 3) / 2 + 1;
    a.Wo = ceil ? ceil_pool_out(Wi) : (Wi - 3) / 2 + 1;
    const int64_t tin = (int64_t)S * Hi * Wi * C, tout = (int64_t)S * a.Ho * a.Wo * C;
    if (tin >= (1ll << 40) || (tin + 255) / 256 >= (1ll << 31)) return SA_EINVAL;
    a.total = (uint64_t)(bwd ? tin : tout);
    return 0;
}

static int pool_fwd(const void* x, int dtype, void* y, void* idx, int S, int Hi, int Wi, int C, bool ceil, void* stream) {
    if (!x || !y || !idx) return SA_EINVAL;
    LpPool a = {};
    const int rc = pool_args(a, dtype, S, Hi, Wi, C, ceil, false);
    if (rc) return rc;
    a.x = x; a.y = y; a.idx = (unsigned char*)idx;
    const dim3 grid((unsigned)((a.total + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (ceil && dtype == SA_F32) SA_LAUNCH((lpips_maxpool_fwd_kernel<float, true>), grid, dim3(256), 0, st, a);
    else if (ceil) SA_LAUNCH((lpips_maxpool_fwd_kernel<bf16_t, true>), grid, dim3(256), 0, st, a);
    else if (dtype == SA_F32) SA_LAUNCH((lpips_maxpool_fwd_kernel<float, false>), grid, dim3(256), 0, st, a);
    else SA_LAUNCH((lpips_maxpool_fwd_kernel<bf16_t, false>), grid, dim3(256), 0, st, a);
    SA_CHECK_LAUNCH();
    return 0;
}

static int pool_bwd(const void* gy, const void* idx, const void* addend, const void* mask, int dtype, void* gx, int S, int Hi, int Wi, int C, bool ceil,
                    void* stream) {
    if (!gy || !idx || !gx) return SA_EINVAL;
    LpPool a = {};
    const int rc = pool_args(a, dtype, S, Hi, Wi, C, ceil, true);
    if (rc) return rc;
    a.gy = gy; a.idx = (unsigned char*)idx; a.addend = addend; a.mask = mask; a.gx = gx;
    LP_LAUNCH_T(dtype, lpips_maxpool_bwd_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}

}  // namespace sa

extern "C" int sa_lpips_unfold(const float* x, int dtype, void* cols, const int32_t* slice_ids, int S, int view, int B, int D, int H, int W, int normalize,
                               int ld, void* stream) {
    using namespace sa;
    if (!x || !cols || !slice_ids) return SA_EINVAL;
    if (dtype != SA_F32 && dtype != SA_BF16) return SA_EUNSUPPORTED;
    LpUnfold a = {};
    if (S <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0 || !make_view(view, D, H, W, a.v)) return SA_EINVAL;
    const int sz = dtype == SA_F32 ? 4 : 2;
    if (ld < LP_TAPS + LP_CLS || ((int64_t)ld * sz) % 16 || (int64_t)ld * sz / 16 > 256) return SA_EINVAL;
    if (a.v.h < LP_K - 2 * LP_P || a.v.w < LP_K - 2 * LP_P) return SA_EINVAL;
    a.ho = conv1_out(a.v.h); a.wo = conv1_out(a.v.w);
    const int64_t rows = (int64_t)S * a.ho * a.wo;
    if (!lp_ok(rows) || !lp_ok((int64_t)B * D * H * W) || !lp_ok((int64_t)B * a.v.n)) return SA_EINVAL;
    a.x = x; a.cols = cols; a.ids = slice_ids;
    a.S = S; a.B = B; a.ld = ld; a.normalize = normalize;
    a.rows = (uint32_t)rows;
    a.chunks = (uint32_t)((int64_t)ld * sz / 16);
    a.rpb = 256u / a.chunks;
    a.dWo = make_fastdiv((uint32_t)a.wo); a.dHo = make_fastdiv((uint32_t)a.ho); a.dCh = make_fastdiv(a.chunks);
    uint64_t blocks = ((uint64_t)rows + a.rpb - 1) / a.rpb;
    if (blocks > 16384u) blocks = 16384u;
    LP_LAUNCH_T(dtype, lpips_unfold_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_lpips_fold(const float* dcols, float* grad, const int32_t* slice_ids, int S, int view, int B, int D, int H, int W, float scale, int ld,
                             void* stream) {
    using namespace sa;
    if (!dcols || !grad || !slice_ids) return SA_EINVAL;
    LpFold a = {};
    if (S <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0 || !make_view(view, D, H, W, a.v)) return SA_EINVAL;
    if (ld < LP_TAPS || a.v.h < LP_K - 2 * LP_P || a.v.w < LP_K - 2 * LP_P) return SA_EINVAL;
    a.ho = conv1_out(a.v.h); a.wo = conv1_out(a.v.w);
    const int64_t total = (int64_t)S * a.v.h * a.v.w;
    if (!lp_ok(total) || !lp_ok((int64_t)B * D * H * W) || !lp_ok((int64_t)B * a.v.n) || !lp_ok((int64_t)S * a.ho * a.wo)) return SA_EINVAL;
    a.dcols = dcols; a.grad = grad; a.ids = slice_ids;
    a.S = S; a.B = B; a.ld = ld; a.scale = scale;
    a.total = (uint32_t)total;
    a.dW = make_fastdiv((uint32_t)a.v.w); a.dH = make_fastdiv((uint32_t)a.v.h);
    SA_LAUNCH(lpips_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_lpips_maxpool_fwd(const void* x, int dtype, void* y, void* idx, int S, int Hi, int Wi, int C, void* stream) {
    return sa::pool_fwd(x, dtype, y, idx, S, Hi, Wi, C, false, stream);
}

extern "C" int sa_lpips_maxpool_bwd(const void* gy, const void* idx, const void* addend, const void* mask, int dtype, void* gx, int S, int Hi, int Wi, int C,
                                    void* stream) {
    return sa::pool_bwd(gy, idx, addend, mask, dtype, gx, S, Hi, Wi, C, false, stream);
}

extern "C" int sa_lpips_maxpool_ceil_fwd(const void* x, int dtype, void* y, void* idx, int S, int Hi, int Wi, int C, void* stream) {
    return sa::pool_fwd(x, dtype, y, idx, S, Hi, Wi, C, true, stream);
}

extern "C" int sa_lpips_maxpool_ceil_bwd(const void* gy, const void* idx, const void* addend, const void* mask, int dtype, void* gx, int S, int Hi, int Wi,
                                         int C, void* stream) {
    return sa::pool_bwd(gy, idx, addend, mask, dtype, gx, S, Hi, Wi, C, true, stream);
}

extern "C" int sa_lpips_head(const void* f0, const void* f1, int dtype, const float* w, int S, int P, int C, float* d, void* g1, int relu_mask, void* stream) {
    using namespace sa;
    if (!f0 || !f1 || !w || !d) return SA_EINVAL;
    if (dtype != SA_F32 && dtype != SA_BF16) return SA_EUNSUPPORTED;
    if (S <= 0 || P <= 0 || C <= 0 || C > LP_MAXC) return SA_EINVAL;
    if (!lp_ok((int64_t)S) || (int64_t)S * P * C >= (1ll << 40)) return SA_EINVAL;
    LpHead a = {};
    a.f0 = f0; a.f1 = f1; a.w = w; a.d = d; a.g1 = g1;
    a.P = P; a.C = C; a.relu_mask = relu_mask;
    a.inv_p = 1.f / (float)P;
    LP_LAUNCH_T(dtype, lpips_head_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}
