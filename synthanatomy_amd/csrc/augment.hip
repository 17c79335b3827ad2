// Training augmentations of the VQ-VAE data path (reference src/utils/vqvae.py:183-371: RandSpatialCropd / RandFlipd / RandRotate90d or RandAffined, then
// RandAdjustContrastd, RandShiftIntensityd, RandGaussianNoised and the two ThresholdIntensityd) on volumes that already sit on the device: sa_augment.
//
// x [B, 1, Di, Hi, Wi] fp32 -> y [B, 1, Do, Ho, Wo] fp32, one sa_augment_params record per sample (include/synthanatomy_hip.h).  Axis 0 = D, 1 = H, 2 = W.
// Two launches on the caller's stream, no host synchronisation:
//   pass 1  spatial stage; samples WITHOUT the gamma bit also get their intensity stage here and are finished.  Samples with the gamma bit are written
//           as they come out of the spatial stage and their minimum / maximum are reduced (wave shuffle -> LDS -> one atomic pair per block).
//   pass 2  samples with the gamma bit only: the intensity stage in place, with the finished minimum / maximum.
// Spatial stage of output voxel o = (d, h, w):
//   IDENTITY     y[o] = x[off + o]
//   SIGNED_PERM  c_a = sign[a] > 0 ? o_a : n_out[a] - 1 - o_a;  source axis perm[a] gets off[perm[a]] + c_a  (an exact gather: crop at off, then flips / rot90s)
//   AFFINE       p = M . [o - c_out; 1] + c_win, c_out = (n_out - 1) / 2, c_win = (ext - 1) / 2: a position inside the source window [off, off + ext)
//                (align_corners = True on the centred voxel grid, MONAI Resample); fp32, evaluated left to right without contraction.  Trilinear over the
//                eight corners floor(p) + {0, 1}^3, a corner outside the window counts as 0 (padding_mode = "zeros").
//   All three gathers of the first two modes are one affine index map  base + d s0 + h s1 + w s2  whose coefficients are uniform per sample.
// Intensity stage, in the reference's order (each step behind its bit of `flags`):
//   gamma  t = (v - min) / ((max - min) + 1e-7f);  v = powf(t, gamma) * (max - min) + min     (min / max of the sample after the spatial stage)
//   shift  v += shift
//   noise  v += noise_std * n(e)
//   clamp  v = min(max(v, 0), 1)
// Noise n(e), e = the voxel's flat index inside its sample's output (d * Ho * Wo + h * Wo + w), q = e >> 2:
//   (w0, w1, w2, w3) = Philox4x32-10(counter = { lo32(q), hi32(q), sample index b, 0 }, key = { lo32(seed), hi32(seed) })     (csrc/dropout.h)
//   u_k = (float(w_k >> 8) + 0.5f) * 2^-24   in fp32 (so u in (0, 1]: log(0) cannot occur; w >> 8 >= 2^23 rounds to even in the addition)
//   r = sqrtf(-2 * logf(u_0)), a = 6.2831853071795864769f * u_1:  n(4q) = r * cosf(a), n(4q + 1) = r * sinf(a);  the same with (u_2, u_3) for 4q + 2, 4q + 3.
// Minimum / maximum: order-free atomicMax on 64-bit words  (call epoch << 32) | image, image = the order-preserving unsigned image of the float
// (inverted for the minimum).  The epoch is a process-wide call counter, so words left by earlier calls lose every comparison and the workspace never
// needs clearing; it must be ZERO when it is first used.  Negative input is fine (the image orders all finite floats).
#include "dropout.h"

namespace sa {

struct AugGeom {
    int Di, Hi, Wi, Do, Ho, Wo;
    int64_t nin, nout;      // voxels per sample
    uint32_t ngroups;       // (nout + 3) / 4
    FastDiv dHW, dW;        // / (Ho * Wo), / Wo
    uint32_t k0, k1;        // Philox key
    uint32_t epoch;
};

__device__ __forceinline__ uint32_t ordered_image(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// per-sample state, uniform over the block
struct AugSample {
    int mode, flags, ok;
    int64_t base, s0, s1, s2;    // gather index map (IDENTITY, SIGNED_PERM)
    int off0, off1, off2, ext0, ext1, ext2;
    float gamma, shift, std;
};

__device__ __forceinline__ int64_t in_stride(int axis, const AugGeom& g) { return axis == 0 ? (int64_t)g.Hi * g.Wi : axis == 1 ? (int64_t)g.Wi : 1; }
__device__ __forceinline__ int in_dim(int axis, const AugGeom& g) { return axis == 0 ? g.Di : axis == 1 ? g.Hi : g.Wi; }

__device__ __forceinline__ AugSample load_sample(const sa_augment_params& p, const AugGeom& g) {
    AugSample s;
    s.mode = p.mode;
    s.flags = p.flags;
    s.gamma = p.gamma;
    s.shift = p.shift;
    s.std = p.noise_std;
    s.off0 = p.off[0]; s.off1 = p.off[1]; s.off2 = p.off[2];
    s.ext0 = p.ext[0]; s.ext1 = p.ext[1]; s.ext2 = p.ext[2];
    s.base = 0; s.s0 = 0; s.s1 = 0; s.s2 = 0;
    s.ok = 1;
    if (s.mode == SA_AUG_AFFINE) {
        s.ok = s.off0 >= 0 && s.off1 >= 0 && s.off2 >= 0 && s.ext0 >= 1 && s.ext1 >= 1 && s.ext2 >= 1 &&
               (int64_t)s.off0 + s.ext0 <= g.Di && (int64_t)s.off1 + s.ext1 <= g.Hi && (int64_t)s.off2 + s.ext2 <= g.Wi;
    } else if (s.mode == SA_AUG_IDENTITY || s.mode == SA_AUG_SIGNED_PERM) {
        const bool sp = s.mode == SA_AUG_SIGNED_PERM;
        const int p0 = sp ? p.perm[0] : 0, p1 = sp ? p.perm[1] : 1, p2 = sp ? p.perm[2] : 2;
        const bool perm_ok = p0 >= 0 && p0 < 3 && p1 >= 0 && p1 < 3 && p2 >= 0 && p2 < 3 && p0 != p1 && p0 != p2 && p1 != p2;
        if (!perm_ok) {
            s.ok = 0;
        } else {
            const int n[3] = {g.Do, g.Ho, g.Wo};
            const int pa[3] = {p0, p1, p2};
            int64_t st[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int k = pa[a];
                const int o = k == 0 ? s.off0 : k == 1 ? s.off1 : s.off2;
                if (o < 0 || (int64_t)o + n[a] > in_dim(k, g)) s.ok = 0;
                const int64_t str = in_stride(k, g);
                const bool neg = sp && p.sign[a] < 0;
                s.base += (int64_t)o * str + (neg ? (int64_t)(n[a] - 1) * str : 0);
                st[a] = neg ? -str : str;
            }
            s.s0 = st[0]; s.s1 = st[1]; s.s2 = st[2];
        }
    } else {
        s.ok = 0;
    }
    return s;
}

// one corner of the trilinear stencil: window-relative index (i0, i1, i2), 0 outside the window
__device__ __forceinline__ float aug_corner(const float* __restrict__ xb, const AugSample& s, const AugGeom& g, int i0, int i1, int i2) {
    if (i0 < 0 || i0 >= s.ext0 || i1 < 0 || i1 >= s.ext1 || i2 < 0 || i2 >= s.ext2) return 0.f;
    return xb[((int64_t)(s.off0 + i0) * g.Hi + (s.off1 + i1)) * g.Wi + (s.off2 + i2)];
}

__device__ __forceinline__ float aug_affine(const float* __restrict__ xb, const float* __restrict__ M, const AugSample& s, const AugGeom& g, int d, int h,
                                            int w) {
    const float dd = (float)d - 0.5f * (float)(g.Do - 1), dh = (float)h - 0.5f * (float)(g.Ho - 1), dw = (float)w - 0.5f * (float)(g.Wo - 1);
    const float p0 = M[0] * dd + M[1] * dh + M[2] * dw + M[3] + 0.5f * (float)(s.ext0 - 1);
    const float p1 = M[4] * dd + M[5] * dh + M[6] * dw + M[7] + 0.5f * (float)(s.ext1 - 1);
    const float p2 = M[8] * dd + M[9] * dh + M[10] * dw + M[11] + 0.5f * (float)(s.ext2 - 1);
    // every corner outside the window (also NaN / inf positions): exactly 0, and the int conversions below stay in range
    if (!(p0 > -1.f && p0 < (float)s.ext0 && p1 > -1.f && p1 < (float)s.ext1 && p2 > -1.f && p2 < (float)s.ext2)) return 0.f;
    const float f0 = floorf(p0), f1 = floorf(p1), f2 = floorf(p2);
    const float t0 = p0 - f0, t1 = p1 - f1, t2 = p2 - f2;
    const int i0 = (int)f0, i1 = (int)f1, i2 = (int)f2;
    const float a0 = 1.f - t0, a1 = 1.f - t1, a2 = 1.f - t2;
    float v = aug_corner(xb, s, g, i0, i1, i2) * (a0 * a1 * a2);
    v += aug_corner(xb, s, g, i0, i1, i2 + 1) * (a0 * a1 * t2);
    v += aug_corner(xb, s, g, i0, i1 + 1, i2) * (a0 * t1 * a2);
    v += aug_corner(xb, s, g, i0, i1 + 1, i2 + 1) * (a0 * t1 * t2);
    v += aug_corner(xb, s, g, i0 + 1, i1, i2) * (t0 * a1 * a2);
    v += aug_corner(xb, s, g, i0 + 1, i1, i2 + 1) * (t0 * a1 * t2);
    v += aug_corner(xb, s, g, i0 + 1, i1 + 1, i2) * (t0 * t1 * a2);
    v += aug_corner(xb, s, g, i0 + 1, i1 + 1, i2 + 1) * (t0 * t1 * t2);
    return v;
}

// the four normals of group q of sample b
__device__ __forceinline__ void aug_normals4(const AugGeom& g, uint32_t b, uint64_t q, float (&n)[4]) {
    const Philox4 w = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), b, 0u, g.k0, g.k1);
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const float u0 = ((float)(w.v[k] >> 8) + 0.5f) * 5.9604644775390625e-8f, u1 = ((float)(w.v[k + 1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
        const float r = sqrtf(-2.f * logf(u0)), a = 6.2831853071795864769f * u1;
        n[k] = r * cosf(a);
        n[k + 1] = r * sinf(a);
    }
}

__device__ __forceinline__ float aug_intensity(float v, const AugSample& s, float mn, float rng, float n) {
    if (s.flags & SA_AUG_GAMMA) v = powf((v - mn) / (rng + 1e-7f), s.gamma) * rng + mn;
    if (s.flags & SA_AUG_SHIFT) v += s.shift;
    if (s.flags & SA_AUG_NOISE) v += s.std * n;
    if (s.flags & SA_AUG_CLAMP) v = fminf(fmaxf(v, 0.f), 1.f);
    return v;
}

// four consecutive output voxels 4q .. 4q + 3 of one sample: one 16-byte store where the address allows it
__device__ __forceinline__ void aug_store4(float* __restrict__ yb, int64_t e0, int64_t nout, const float (&v)[4]) {
    float* p = yb + e0;
    if (e0 + 3 < nout && (((uintptr_t)p) & 15u) == 0) {
        *reinterpret_cast<float4_t*>(p) = float4_t{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (e0 + r < nout) p[r] = v[r];
    }
}

__global__ void __launch_bounds__(256) augment_spatial_kernel(const float* __restrict__ x, float* __restrict__ y, const sa_augment_params* __restrict__ params,
                                                              unsigned long long* __restrict__ ws, const AugGeom g) {
    const uint32_t b = blockIdx.y;
    const sa_augment_params& P = params[b];
    const AugSample s = load_sample(P, g);
    const float* xb = x + (int64_t)b * g.nin;
    float* yb = y + (int64_t)b * g.nout;
    const bool gamma = (s.flags & SA_AUG_GAMMA) != 0;
    float lo = INFINITY, hi = -INFINITY;
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < g.ngroups; q += gridDim.x * 256u) {
        const uint32_t e0 = q * 4u;
        int d = (int)fdiv(e0, g.dHW);
        const uint32_t rem = e0 - (uint32_t)d * (uint32_t)(g.Ho * g.Wo);
        int h = (int)fdiv(rem, g.dW);
        int w = (int)(rem - (uint32_t)h * (uint32_t)g.Wo);
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (!gamma && (s.flags & SA_AUG_NOISE)) aug_normals4(g, b, q, n);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t = 0.f;
            if ((int64_t)e0 + r < g.nout && s.ok) {
                t = s.mode == SA_AUG_AFFINE ? aug_affine(xb, P.M, s, g, d, h, w) : xb[s.base + d * s.s0 + h * s.s1 + w * s.s2];
                if (gamma) {
                    lo = fminf(lo, t);
                    hi = fmaxf(hi, t);
                } else {
                    t = aug_intensity(t, s, 0.f, 0.f, n[r]);
                }
            }
            v[r] = t;
            if (++w == g.Wo) {
                w = 0;
                if (++h == g.Ho) {
                    h = 0;
                    ++d;
                }
            }
        }
        aug_store4(yb, (int64_t)e0, g.nout, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ws[4 * b + 3] = s.ok ? 0ull : 1ull;
    if (!gamma) return;      // (uniform over the block)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    __shared__ float red[8];
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[4 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        if (lo <= hi) {      // (a block without a voxel of its own holds +inf / -inf)
            const unsigned long long ep = (unsigned long long)g.epoch << 32;
            atomicMax(ws + 4 * b, ep | (unsigned long long)(~ordered_image(lo)));
            atomicMax(ws + 4 * b + 1, ep | (unsigned long long)ordered_image(hi));
        }
    }
}

__global__ void __launch_bounds__(256) augment_intensity_kernel(float* __restrict__ y, const sa_augment_params* __restrict__ params,
                                                                unsigned long long* __restrict__ ws, const AugGeom g) {
    const uint32_t b = blockIdx.y;
    const sa_augment_params& P = params[b];
    if (!(P.flags & SA_AUG_GAMMA)) return;      // finished by pass 1
    AugSample s;
    s.flags = P.flags;
    s.gamma = P.gamma;
    s.shift = P.shift;
    s.std = P.noise_std;
    const unsigned long long wlo = ws[4 * b], whi = ws[4 * b + 1];
    // words of another epoch: the sample had no valid voxel (a rejected record) -- nothing to do
    if ((uint32_t)(wlo >> 32) != g.epoch || (uint32_t)(whi >> 32) != g.epoch) return;
    const float mn = ordered_value(~(uint32_t)wlo), mx = ordered_value((uint32_t)whi);
    const float rng = mx - mn;
    if (blockIdx.x == 0 && threadIdx.x == 0) ws[4 * b + 2] = (unsigned long long)__float_as_uint(mn) | ((unsigned long long)__float_as_uint(mx) << 32);
    float* yb = y + (int64_t)b * g.nout;
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < g.ngroups; q += gridDim.x * 256u) {
        const int64_t e0 = (int64_t)q * 4;
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (s.flags & SA_AUG_NOISE) aug_normals4(g, b, q, n);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        float* p = yb + e0;
        if (e0 + 3 < g.nout && (((uintptr_t)p) & 15u) == 0) {
            const float4_t t = *reinterpret_cast<const float4_t*>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (e0 + r < g.nout) v[r] = p[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = aug_intensity(v[r], s, mn, rng, n[r]);
        aug_store4(yb, e0, g.nout, v);
    }
}

static std::atomic<uint32_t> g_augment_epoch{0};

}  // namespace sa

using namespace sa;

extern "C" int64_t sa_augment_workspace_bytes(int B) { return B > 0 ? (int64_t)B * 32 : (int64_t)SA_EINVAL; }

extern "C" int sa_augment(const float* x, float* y, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, const sa_augment_params* params, uint64_t seed,
                          void* ws, void* stream) {
    if (!x || !y || !params || !ws || x == y || B < 1 || B > 65535 || Di < 1 || Hi < 1 || Wi < 1 || Do < 1 || Ho < 1 || Wo < 1) return SA_EINVAL;
    AugGeom g;
    g.Di = Di; g.Hi = Hi; g.Wi = Wi; g.Do = Do; g.Ho = Ho; g.Wo = Wo;
    g.nin = (int64_t)Di * Hi * Wi;
    g.nout = (int64_t)Do * Ho * Wo;
    if (g.nout > 0x7ffffff0ll) return SA_EUNSUPPORTED;      // (the voxel index of a sample's output is split with 32-bit multiply-high divisions)
    g.ngroups = (uint32_t)((g.nout + 3) >> 2);
    g.dHW = make_fastdiv((uint32_t)(Ho * Wo));
    g.dW = make_fastdiv((uint32_t)Wo);
    g.k0 = (uint32_t)seed;
    g.k1 = (uint32_t)(seed >> 32);
    uint32_t ep = g_augment_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
    if (ep == 0) ep = g_augment_epoch.fetch_add(1, std::memory_order_relaxed) + 1;      // (epoch 0 is the cleared workspace)
    g.epoch = ep;
    const dim3 grid((g.ngroups + 255u) / 256u, (unsigned)B);      // one group of four voxels per thread (<= 2^21 blocks per sample)
    SA_LAUNCH(augment_spatial_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, params, (unsigned long long*)ws, g);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(augment_intensity_kernel, grid, dim3(256), 0, (hipStream_t)stream, y, params, (unsigned long long*)ws, g);
    SA_CHECK_LAUNCH();
    return 0;
}
