// One-channel ends of the VQ-VAE for ANY sampling geometry: the first nn.Conv3d(1 -> C) and the last nn.ConvTranspose3d(C -> 1) of the reference
// (src/networks/vqvae/baseline.py:218-226, :283-293) with kernel 1 .. 4, stride 1 or 2, any padding / dilation / output_padding.
//
// With one channel on the volume side the k^3 taps are the whole reduction (first layer) or the whole output (last layer), so both layers are a
// 1x1x1 convolution over cells with the taps as channels (MFMA, csrc/conv_fprop.hip) between two memory-bound rearrangements:
//   sa_taps_unfold : Xc[n][m][t] = x[n][m * mult + t * step + off] per axis (zero outside), t = (td * k + th) * k + tw   -- im2col of a volume onto a grid
//                    of cells: the first layer's forward (mult = stride, step = dilation, off = -padding) and the last layer's backward (the same
//                    three numbers, the volume being the output gradient); optionally db += sum of the volume (the last layer's bias gradient)
//   sa_taps_fold   : out[n][o] = bias + sum over taps t with (o + pad - t * dil) divisible by the stride of P[n][(o + pad - t * dil) / stride][t]
//                    -- the last layer's forward, a GATHER per output voxel: no atomics, one fixed summation order, bitwise reproducible; output voxels no
//                    tap reaches (output_padding planes) get the bias
// csrc/convt1.hip keeps the kernels specialised for k4 s2 p1 (sa_convt1_im2col / sa_convt1_gather); these take every other tuple.
#include "sa_common.h"

namespace sa {

struct TapsUnfold {
    const float* x;     // [N, Di, Hi, Wi] fp32
    void* xc;           // [N, Dm, Hm, Wm, ld] T
    float* db;          // += sum x, or NULL
    int32_t N, Di, Hi, Wi, Dm, Hm, Wm;
    int32_t mult, step, off, ld;
    uint32_t cells, chunks, cpb;   // rows; 16-byte chunks per row; rows per block pass (256 / chunks)
    uint64_t nvox;
    FastDiv dW_, dH_, dD_, dCh_;
};

// thread = (cell, 16-byte chunk of its row): a block writes `cpb` consecutive rows, i.e. one contiguous range, 16 bytes per lane; the volume is
// 1 / k^3 .. 1 / (k/s)^3 of the traffic and every voxel is read by neighbouring lanes of the same block (L1 / L2 hits).
template <typename T, int K>
__global__ __launch_bounds__(256) void taps_unfold_kernel(const TapsUnfold a) {
    constexpr int VEC = 16 / (int)sizeof(T), T3 = K * K * K;
    const uint32_t tid = threadIdx.x;
    const uint32_t lc = fdiv(tid, a.dCh_), ch = tid - lc * a.chunks;
    if (lc < a.cpb) {
        for (uint32_t cell = blockIdx.x * a.cpb + lc; cell < a.cells; cell += gridDim.x * a.cpb) {
            uint32_t q = fdiv(cell, a.dW_);
            const int mw = (int)(cell - q * (uint32_t)a.Wm);
            uint32_t q2 = fdiv(q, a.dH_);
            const int mh = (int)(q - q2 * (uint32_t)a.Hm);
            const int n = (int)fdiv(q2, a.dD_);
            const int md = (int)(q2 - (uint32_t)n * (uint32_t)a.Dm);
            const int bd = md * a.mult + a.off, bh = mh * a.mult + a.off, bw = mw * a.mult + a.off;
            const float* vol = a.x + (int64_t)n * a.Di * a.Hi * a.Wi;
            float v[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const uint32_t t = ch * VEC + e;
                const int td = (int)(t / (K * K)), th = (int)((t / K) % K), tw = (int)(t % K);
                const int id = bd + td * a.step, ih = bh + th * a.step, iw = bw + tw * a.step;
                const bool ok = t < (uint32_t)T3 && (unsigned)id < (unsigned)a.Di && (unsigned)ih < (unsigned)a.Hi && (unsigned)iw < (unsigned)a.Wi;
                v[e] = ok ? vol[((int64_t)id * a.Hi + ih) * a.Wi + iw] : 0.f;
            }
            unsigned char* dst = (unsigned char*)a.xc + ((size_t)cell * a.ld) * sizeof(T) + (size_t)ch * 16;
            if constexpr (sizeof(T) == 4) {
                *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                uint4 pk;
                pk.x = pack2<T>(v[0], v[1]);
                pk.y = pack2<T>(v[2], v[3]);
                pk.z = pack2<T>(v[4], v[5]);
                pk.w = pack2<T>(v[6], v[7]);
                *(uint4*)dst = pk;
            }
        }
    }
    if (a.db) {   // (block-uniform) the bias gradient of the last layer: every voxel of the volume once, whether a window reads it or not
        float gsum = 0.f;
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + tid; i < a.nvox; i += (uint64_t)gridDim.x * 256u) gsum += a.x[i];
        __shared__ float red[4];
        gsum = wave_sum(gsum);
        if ((tid & 63u) == 0) red[tid >> 6] = gsum;
        __syncthreads();
        if (tid == 0) unsafeAtomicAdd(a.db, red[0] + red[1] + red[2] + red[3]);
    }
}

struct TapsFold {
    const float* p;     // [N, Dc, Hc, Wc, ld] fp32
    const float* bias;  // [1] or NULL
    float* out;         // [N, Do, Ho, Wo] fp32
    int32_t N, Dc, Hc, Wc, Do, Ho, Wo;
    int32_t pad, dil, ld;
    uint32_t nwt, nht, ndt;
};

// per axis: (applies, cell) of output o and tap t
template <int S>
__device__ __forceinline__ bool fold_cell(int o, int t, int pad, int dil, int C, int& q) {
    const int nmr = o + pad - t * dil;
    if (S == 2 && (nmr & 1)) return false;
    q = S == 2 ? nmr >> 1 : nmr;          // (exact: nmr is even; arithmetic shift for negative values)
    return (unsigned)q < (unsigned)C;
}

// A block = a 3-D tile of 4 (od) x 8 (oh) x 16 (ow) outputs, thread = two neighbours along W (the layout of convt1_gather_kernel): the P rows a tile touches
// are touched by its own threads and the halo of its neighbours only, so fetched lines are used whole.  Taps in the order td, th, tw: one fixed sum per voxel.
template <int K, int S>
__global__ __launch_bounds__(256) void taps_fold_kernel(const TapsFold a) {
    const float b = a.bias ? a.bias[0] : 0.f;
    uint32_t t = blockIdx.x;
    const uint32_t wt = t % a.nwt; t /= a.nwt;
    const uint32_t ht = t % a.nht; t /= a.nht;
    const uint32_t dt = t % a.ndt;
    const int n = (int)(t / a.ndt);
    const int ow = (int)(wt * 8 + (threadIdx.x & 7u)) * 2, oh = (int)(ht * 8 + ((threadIdx.x >> 3) & 7u)), od = (int)(dt * 4 + (threadIdx.x >> 6));
    if (ow >= a.Wo || oh >= a.Ho || od >= a.Do) return;
    float s0 = b, s1 = b;
#pragma unroll
    for (int td = 0; td < K; ++td) {
        int qd;
        if (!fold_cell<S>(od, td, a.pad, a.dil, a.Dc, qd)) continue;
#pragma unroll
        for (int th = 0; th < K; ++th) {
            int qh;
            if (!fold_cell<S>(oh, th, a.pad, a.dil, a.Hc, qh)) continue;
            const float* row = a.p + ((((int64_t)n * a.Dc + qd) * a.Hc + qh) * a.Wc) * a.ld + (td * K + th) * K;
#pragma unroll
            for (int tw = 0; tw < K; ++tw) {
                int q0, q1;
                if (fold_cell<S>(ow, tw, a.pad, a.dil, a.Wc, q0)) s0 += row[(int64_t)q0 * a.ld + tw];
                if (fold_cell<S>(ow + 1, tw, a.pad, a.dil, a.Wc, q1)) s1 += row[(int64_t)q1 * a.ld + tw];
            }
        }
    }
    const int64_t o = (((int64_t)n * a.Do + od) * a.Ho + oh) * a.Wo + ow;
    if (ow + 1 < a.Wo && (o & 1) == 0) {
        *(float2*)(a.out + o) = make_float2(s0, s1);
    } else {
        a.out[o] = s0;
        if (ow + 1 < a.Wo) a.out[o + 1] = s1;
    }
}

template <typename T, int K>
static void launch_unfold(const TapsUnfold& a, unsigned blocks, hipStream_t st, const char* tn) {
    char name[64];
    snprintf(name, sizeof name, "taps_unfold_kernel<%s, %d>", tn, K);
    note_kernel(name);
    hipLaunchKernelGGL((taps_unfold_kernel<T, K>), dim3(blocks), dim3(256), 0, st, a);
}

template <typename T>
static void launch_unfold_k(const TapsUnfold& a, int k, unsigned blocks, hipStream_t st, const char* tn) {
    switch (k) {
        case 1: launch_unfold<T, 1>(a, blocks, st, tn); break;
        case 2: launch_unfold<T, 2>(a, blocks, st, tn); break;
        case 3: launch_unfold<T, 3>(a, blocks, st, tn); break;
        default: launch_unfold<T, 4>(a, blocks, st, tn); break;
    }
}

template <int K, int S>
static void launch_fold(const TapsFold& a, unsigned blocks, hipStream_t st) {
    char name[64];
    snprintf(name, sizeof name, "taps_fold_kernel<%d, %d>", K, S);
    note_kernel(name);
    hipLaunchKernelGGL((taps_fold_kernel<K, S>), dim3(blocks), dim3(256), 0, st, a);
}

template <int S>
static void launch_fold_k(const TapsFold& a, int k, unsigned blocks, hipStream_t st) {
    switch (k) {
        case 1: launch_fold<1, S>(a, blocks, st); break;
        case 2: launch_fold<2, S>(a, blocks, st); break;
        case 3: launch_fold<3, S>(a, blocks, st); break;
        default: launch_fold<4, S>(a, blocks, st); break;
    }
}

static bool taps_extent_ok(int64_t v) { return v > 0 && v < (1ll << 31) - 16; }

}  // namespace sa

extern "C" int sa_taps_unfold(const float* x, int dtype, void* xc, float* db, int N, int Di, int Hi, int Wi, int Dm, int Hm, int Wm, int k, int mult, int step,
                              int off, int ld, void* stream) {
    using namespace sa;
    if (!x || !xc) return SA_EINVAL;
    if (dtype != SA_F32 && dtype != SA_BF16 && dtype != SA_F16) return SA_EUNSUPPORTED;
    if (k < 1 || k > 4) return SA_EUNSUPPORTED;
    const int sz = dtype == SA_F32 ? 4 : 2;
    if (N <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0 || Dm <= 0 || Hm <= 0 || Wm <= 0 || mult < 1 || step < 1) return SA_EINVAL;
    if (ld < k * k * k || ((int64_t)ld * sz) % 16) return SA_EINVAL;
    const int64_t nvox = (int64_t)N * Di * Hi * Wi, cells = (int64_t)N * Dm * Hm * Wm;
    const int64_t chunks = (int64_t)ld * sz / 16;
    // the largest coordinate a thread forms: (Xm - 1) * mult + (k - 1) * step + off, and its negative end `off`
    const int mx = Dm > Hm ? (Dm > Wm ? Dm : Wm) : (Hm > Wm ? Hm : Wm);
    const int64_t reach = (int64_t)(mx - 1) * mult + (int64_t)(k - 1) * step + (off > 0 ? off : -(int64_t)off);
    if (!taps_extent_ok(nvox) || !taps_extent_ok(cells) || !taps_extent_ok(reach + 1) || chunks > 256) return SA_EINVAL;
    TapsUnfold a = {};
    a.x = x; a.xc = xc; a.db = db;
    a.N = N; a.Di = Di; a.Hi = Hi; a.Wi = Wi; a.Dm = Dm; a.Hm = Hm; a.Wm = Wm;
    a.mult = mult; a.step = step; a.off = off; a.ld = ld;
    a.cells = (uint32_t)cells;
    a.chunks = (uint32_t)chunks;
    a.cpb = 256u / a.chunks;
    a.nvox = (uint64_t)nvox;
    a.dW_ = make_fastdiv((uint32_t)Wm); a.dH_ = make_fastdiv((uint32_t)Hm); a.dD_ = make_fastdiv((uint32_t)Dm); a.dCh_ = make_fastdiv(a.chunks);
    uint64_t blocks = ((uint64_t)cells + a.cpb - 1) / a.cpb;
    if (blocks > 8192u) blocks = 8192u;     // grid-stride rows; with db: one atomic per block
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SA_F32) launch_unfold_k<float>(a, k, (unsigned)blocks, st, "float");
    else if (dtype == SA_BF16) launch_unfold_k<bf16_t>(a, k, (unsigned)blocks, st, "unsigned short");
    else launch_unfold_k<f16_t>(a, k, (unsigned)blocks, st, "f16_t");
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_taps_fold(const float* p, const float* bias, float* out, int N, int Dc, int Hc, int Wc, int Do, int Ho, int Wo, int k, int stride, int pad,
                            int dil, int ld, void* stream) {
    using namespace sa;
    if (!p || !out) return SA_EINVAL;
    if (k < 1 || k > 4 || stride < 1 || stride > 2) return SA_EUNSUPPORTED;
    if (N <= 0 || Dc <= 0 || Hc <= 0 || Wc <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0 || pad < 0 || dil < 1) return SA_EINVAL;
    if (ld < k * k * k || ld % 4) return SA_EINVAL;
    const int mo = Do > Ho ? (Do > Wo ? Do : Wo) : (Ho > Wo ? Ho : Wo);
    const int64_t reach = (int64_t)mo + 1 + pad + (int64_t)(k - 1) * dil;
    if (!taps_extent_ok((int64_t)N * Dc * Hc * Wc) || !taps_extent_ok((int64_t)N * Do * Ho * Wo) || !taps_extent_ok(reach)) return SA_EINVAL;
    TapsFold a = {};
    a.p = p; a.bias = bias; a.out = out;
    a.N = N; a.Dc = Dc; a.Hc = Hc; a.Wc = Wc; a.Do = Do; a.Ho = Ho; a.Wo = Wo;
    a.pad = pad; a.dil = dil; a.ld = ld;
    a.nwt = ((uint32_t)Wo + 15u) / 16u; a.nht = ((uint32_t)Ho + 7u) / 8u; a.ndt = ((uint32_t)Do + 3u) / 4u;
    const uint64_t blocks = (uint64_t)N * a.ndt * a.nht * a.nwt;
    if (blocks >= (1ull << 31)) return SA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (stride == 1) launch_fold_k<1>(a, k, (unsigned)blocks, st);
    else launch_fold_k<2>(a, k, (unsigned)blocks, st);
    SA_CHECK_LAUNCH();
    return 0;
}
