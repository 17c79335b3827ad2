// SpectralLoss, HartleyLoss and WaveGANLoss of the reference (src/losses/vqvae/vqvae.py:188-323, 326-519, 641-771; --loss=spectral | hartley |
// wavegan): the spectral terms and d loss / d spectrum over the HALF spectra of pred and target.
//
// Input: Xp, Xy = the UNNORMALISED rfftn of pred and y over (C, D, H, W), [B, C, D, H, W/2 + 1] complex64 (interleaved re, im).  The ortho spectra
// the reference compares are Y = s X with s = 1 / sqrt(C D H W); s is folded in here.  A full-spectrum sum is the half-spectrum sum weighted by the
// bin's multiplicity m (1 on the planes k_W = 0 and, W even, k_W = W/2; 2 elsewhere).  n = B C D H W.  A, phi = |Y|, atan2(Im Y, Re Y).
//   spectral: sums = (sum m (Ap - Ay)^2, sum m (1 - e^|dphi|)^2, 0), dphi = phi_p - phi_y unwrapped in (-2 pi, 2 pi)
//             g = (Ap - Ay)/n * u + (e^|dphi| - 1) e^|dphi| sign(dphi) / (n Ap) * i u,  u = Yp / Ap
//   hartley:  sums = (sum m w^2 |Yp - Yy|^2, 0, 0), g = w^2 (Yp - Yy) / n; w = 1, or (prioritise_hf) the reference's weight
//             (exp(q) - exp(qmin)) / (exp(qmax) - exp(qmin)) + 1e-4, q = sum over (D, H, W) of (|m_a/2 - i_a| / (m_a/2))^2, min / max separable
//   wavegan:  sums = (sum m (Ay - Ap)^2, sum m Ay^2, sum m |log Ay - log Ap|); a second pass, after the sums are final, writes
//             g = [(Ap - Ay) / (S N) - sign(log Ay - log Ap) / (n Ap)] u,  S = sqrt(sums[0]), N = sqrt(sums[1])
// grad = factor * s * g: the Hermitian part of the full-spectrum gradient (torch's d loss / d Re + i d loss / d Im) on the stored half, so that
// irfftn(grad, norm="forward") over (C, D, H, W) is d loss / d pred.  On the self-conjugate bins (every transformed index 0 or m/2) the spectrum is
// real: Im is forced to +0 before atan2 (the reference's CPU fftn gives +0 there, so phi = pi for a negative real part; rocFFT may leave noise of either
// sign, which would move dphi by 2 pi) and grad's imaginary part is 0 there.  Where |Xp| = 0, u = 0 (the reference's gradient is NaN there).
//
// One thread per bin in a grid-stride loop over a grid that depends on the shape only; each block leaves three fp64 partials and a single block sums
// them in a fixed order -- no atomics, so sums and grad are bitwise reproducible.  grad may alias Xp (each thread reads its bin before writing it).
#include "sa_common.h"

namespace sa {

constexpr int FL_THREADS = 256;
constexpr int FL_MAX_BLOCKS = 2048;

struct FourierGeom {
    uint32_t nbins;
    int C, D, H, W, Wh;
    FastDiv fWh, fH, fD, fC;
    float s;           // 1 / sqrt(C D H W)
    float inv_n;       // 1 / (B C D H W)
    float gscale;      // factor * s
    float emin, inv_erange;            // hartley: exp(qmin), 1 / (exp(qmax) - exp(qmin)); qmin is separable, qmax = 3 (every i_a = 0)
};

static int fl_blocks(uint32_t nbins) {
    const uint32_t b = (nbins + FL_THREADS - 1) / FL_THREADS;
    return (int)(b < (uint32_t)FL_MAX_BLOCKS ? b : FL_MAX_BLOCKS);
}

// min over i in [0, m) of (|m/2 - i| / (m/2))^2 (fp64, as the reference's numpy.fromfunction): 0 for even m, (1/m)^2 for odd m
static double hartley_axis_min(int m) {
    double best = 1e300;
    for (int i = 0; i < m; ++i) {
        const double t = std::fabs(m / 2.0 - i) / (m / 2.0);
        best = t * t < best ? t * t : best;
    }
    return best;
}

__device__ __forceinline__ float hartley_axis(int i, int m) {
    const float h = 0.5f * (float)m, t = fabsf(h - (float)i) / h;
    return t * t;
}

__device__ __forceinline__ float sgnf_fl(float x) { return (float)((x > 0.f) - (x < 0.f)); }

struct Bin {
    bool self_conj;
    float mult;
    int d, h, kw;
};

__device__ __forceinline__ Bin bin_of(uint32_t i, const FourierGeom& g) {
    Bin b;
    uint32_t r = fdiv(i, g.fWh);
    b.kw = (int)(i - r * (uint32_t)g.Wh);
    uint32_t q = fdiv(r, g.fH);
    b.h = (int)(r - q * (uint32_t)g.H);
    r = fdiv(q, g.fD);
    b.d = (int)(q - r * (uint32_t)g.D);
    q = fdiv(r, g.fC);
    const int c = (int)(r - q * (uint32_t)g.C);
    const bool edge_w = b.kw == 0 || 2 * b.kw == g.W;
    b.mult = edge_w ? 1.f : 2.f;
    b.self_conj = edge_w && (c == 0 || 2 * c == g.C) && (b.d == 0 || 2 * b.d == g.D) && (b.h == 0 || 2 * b.h == g.H);
    return b;
}

__device__ __forceinline__ float2 load_bin(const float2* p, uint32_t i, bool self_conj) {
    float2 v = p[i];
    if (self_conj) v.y = 0.f;
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ws[k * nblk + block] = the block's partial of sums[k]
__device__ __forceinline__ void block_partials(double a0, double a1, double a2, double* __restrict__ ws, int nblk) {
    __shared__ double red[3][FL_THREADS / 64];
    const int tid = threadIdx.x;
    a0 = wave_sum_d(a0);
    a1 = wave_sum_d(a1);
    a2 = wave_sum_d(a2);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = a0;
        red[1][tid >> 6] = a1;
        red[2][tid >> 6] = a2;
    }
    __syncthreads();
    if (tid < 3) ws[(int64_t)tid * nblk + blockIdx.x] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// Pass 1.  KIND 0 spectral, 1 hartley (both also write grad when GRAD), 2 wavegan (sums only).  xp and grad may alias: no __restrict__ on them.
template <int KIND, bool GRAD, bool HF>
__global__ __launch_bounds__(FL_THREADS) void fourier_loss_kernel(const float2* xp, const float2* __restrict__ xy, FourierGeom g, float2* grad,
                                                                  double* __restrict__ ws) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const uint32_t stride = gridDim.x * FL_THREADS;
    for (uint32_t i = blockIdx.x * FL_THREADS + threadIdx.x; i < g.nbins; i += stride) {
        const Bin b = bin_of(i, g);
        const float2 p = load_bin(xp, i, b.self_conj), y = load_bin(xy, i, b.self_conj);
        float2 gr = make_float2(0.f, 0.f);
        if (KIND == 1) {
            float w2 = 1.f;
            if (HF) {
                const float q = hartley_axis(b.d, g.D) + hartley_axis(b.h, g.H) + hartley_axis(b.kw, g.W);
                const float w = (expf(q) - g.emin) * g.inv_erange + 1e-4f;
                w2 = w * w;
            }
            const float dr = (p.x - y.x) * g.s, di = (p.y - y.y) * g.s;
            a0 += (double)(b.mult * w2 * (dr * dr + di * di));
            if (GRAD) {
                const float c = g.gscale * w2 * g.inv_n;
                gr = make_float2(c * dr, c * di);
            }
        } else {
            const float rp = sqrtf(p.x * p.x + p.y * p.y), ry = sqrtf(y.x * y.x + y.y * y.y);
            const float ap = rp * g.s, ay = ry * g.s;
            if (KIND == 0) {
                const float dphi = atan2f(p.y, p.x) - atan2f(y.y, y.x);
                const float e = expf(fabsf(dphi));
                const float da = ap - ay, de = 1.f - e;
                a0 += (double)(b.mult * (da * da));
                a1 += (double)(b.mult * (de * de));
                if (GRAD && rp > 0.f) {
                    const float inv_rp = 1.f / rp;
                    const float ux = p.x * inv_rp, uy = p.y * inv_rp;
                    const float ga = da * g.inv_n;                                       // along u
                    const float gp = (e - 1.f) * e * sgnf_fl(dphi) * g.inv_n / ap;       // along i u
                    gr = make_float2(g.gscale * (ga * ux - gp * uy), g.gscale * (ga * uy + gp * ux));
                }
            } else {
                const float da = ay - ap;
                a0 += (double)(b.mult * (da * da));
                a1 += (double)(b.mult * (ay * ay));
                a2 += (double)(b.mult * fabsf(logf(ay) - logf(ap)));
            }
        }
        if (GRAD) {
            if (b.self_conj) gr.y = 0.f;
            grad[i] = gr;
        }
    }
    block_partials(a0, a1, a2, ws, gridDim.x);
}

// Pass 2 of wavegan: the gradient, with S and N read from the finished sums on the device (no host synchronisation)
__global__ __launch_bounds__(FL_THREADS) void fourier_wavegan_grad_kernel(const float2* xp, const float2* __restrict__ xy, FourierGeom g,
                                                                          const double* __restrict__ sums, float2* grad) {
    const float inv_sn = (float)(1.0 / (sqrt(sums[0]) * sqrt(sums[1])));
    const uint32_t stride = gridDim.x * FL_THREADS;
    for (uint32_t i = blockIdx.x * FL_THREADS + threadIdx.x; i < g.nbins; i += stride) {
        const Bin b = bin_of(i, g);
        const float2 p = load_bin(xp, i, b.self_conj), y = load_bin(xy, i, b.self_conj);
        const float rp = sqrtf(p.x * p.x + p.y * p.y), ry = sqrtf(y.x * y.x + y.y * y.y);
        const float ap = rp * g.s, ay = ry * g.s;
        float2 gr = make_float2(0.f, 0.f);
        if (rp > 0.f) {
            const float inv_rp = 1.f / rp;
            const float ga = g.gscale * ((ap - ay) * inv_sn - sgnf_fl(logf(ay) - logf(ap)) * g.inv_n / ap);
            gr = make_float2(ga * p.x * inv_rp, b.self_conj ? 0.f : ga * p.y * inv_rp);
        }
        grad[i] = gr;
    }
}

// sums[k] = sum over blocks of ws[k * nblk + block], fp64, fixed order (one block)
__global__ __launch_bounds__(FL_THREADS) void fourier_sum_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ sums) {
    __shared__ double red[3][FL_THREADS];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        for (int i = tid; i < nblk; i += FL_THREADS) s += ws[(int64_t)k * nblk + i];
        red[k][tid] = s;
    }
    __syncthreads();
    for (int o = FL_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o)
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
        __syncthreads();
    }
    if (tid < 3) sums[tid] = red[tid][0];
}

}  // namespace sa

using namespace sa;

static bool fourier_shape_ok(int64_t B, int C, int D, int H, int W) {
    return B >= 1 && C >= 1 && D >= 2 && H >= 2 && W >= 2;
}

extern "C" int64_t sa_fourier_loss_workspace_bytes(int64_t B, int C, int D, int H, int W) {
    if (!fourier_shape_ok(B, C, D, H, W)) return SA_EINVAL;
    const int64_t nbins = B * C * D * H * (int64_t)(W / 2 + 1);
    if (nbins > 0x7fffffff) return SA_EUNSUPPORTED;
    return 3 * (int64_t)fl_blocks((uint32_t)nbins) * (int64_t)sizeof(double);
}

extern "C" int sa_fourier_loss(int kind, const float* xp, const float* xy, int64_t B, int C, int D, int H, int W, int prioritise_hf, float factor,
                               double* sums, float* grad, void* ws, void* stream) {
    if (kind < SA_FOURIER_SPECTRAL || kind > SA_FOURIER_WAVEGAN || !xp || !xy || !sums || !ws || !fourier_shape_ok(B, C, D, H, W)) return SA_EINVAL;
    const int64_t nbins = B * C * D * H * (int64_t)(W / 2 + 1);
    if (nbins > 0x7fffffff) return SA_EUNSUPPORTED;
    FourierGeom g;
    g.nbins = (uint32_t)nbins;
    g.C = C; g.D = D; g.H = H; g.W = W; g.Wh = W / 2 + 1;
    g.fWh = make_fastdiv((uint32_t)g.Wh); g.fH = make_fastdiv((uint32_t)H); g.fD = make_fastdiv((uint32_t)D); g.fC = make_fastdiv((uint32_t)C);
    const double vol = (double)C * D * H * W;
    g.s = (float)(1.0 / std::sqrt(vol));
    g.inv_n = (float)(1.0 / ((double)B * vol));
    g.gscale = (float)((double)factor / std::sqrt(vol));
    const double qmin = hartley_axis_min(D) + hartley_axis_min(H) + hartley_axis_min(W);
    g.emin = (float)std::exp(qmin);
    g.inv_erange = (float)(1.0 / (std::exp(3.0) - std::exp(qmin)));

    const int nblk = fl_blocks(g.nbins);
    const float2* p = reinterpret_cast<const float2*>(xp);
    const float2* y = reinterpret_cast<const float2*>(xy);
    float2* gr = reinterpret_cast<float2*>(grad);
    double* w = static_cast<double*>(ws);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), blk(FL_THREADS);
    const bool want = grad != nullptr;
    if (kind == SA_FOURIER_SPECTRAL) {
        if (want) SA_LAUNCH((fourier_loss_kernel<0, true, false>), grid, blk, 0, st, p, y, g, gr, w);
        else SA_LAUNCH((fourier_loss_kernel<0, false, false>), grid, blk, 0, st, p, y, g, gr, w);
    } else if (kind == SA_FOURIER_HARTLEY) {
        if (want && prioritise_hf) SA_LAUNCH((fourier_loss_kernel<1, true, true>), grid, blk, 0, st, p, y, g, gr, w);
        else if (want) SA_LAUNCH((fourier_loss_kernel<1, true, false>), grid, blk, 0, st, p, y, g, gr, w);
        else if (prioritise_hf) SA_LAUNCH((fourier_loss_kernel<1, false, true>), grid, blk, 0, st, p, y, g, gr, w);
        else SA_LAUNCH((fourier_loss_kernel<1, false, false>), grid, blk, 0, st, p, y, g, gr, w);
    } else {
        SA_LAUNCH((fourier_loss_kernel<2, false, false>), grid, blk, 0, st, p, y, g, gr, w);
    }
    SA_CHECK_LAUNCH();
    SA_LAUNCH(fourier_sum_kernel, dim3(1), blk, 0, st, (const double*)w, nblk, sums);
    SA_CHECK_LAUNCH();
    if (kind == SA_FOURIER_WAVEGAN && want) {
        SA_LAUNCH(fourier_wavegan_grad_kernel, grid, blk, 0, st, p, y, g, (const double*)sums, gr);
        SA_CHECK_LAUNCH();
    }
    return 0;
}
