// fp32 / bf16 volume in canonical axes -> NIfTI-1 voxel block as stored, on the device: sa_volume_egress (include/synthanatomy_hip.h).  The
// inverse of sa_volume_ingest (ingest.hip): what the reference leaves to SegmentationSaver(output_ext=".nii.gz", resample=False, dtype=float32)
// (reference run_vqvae.py:467-514) after a host copy of the volume.
//
// x[ext0][ext1][ext2] is last-axis-fastest, the file is axis-0-fastest (offset i0 + n0 (i1 + n1 i2)), n[perm[a]] = ext[a], and file axis perm[a] runs
// backwards along canonical axis a where sign[a] < 0.  On the caller's stream, no host synchronisation:
//   reduce   SA_EGRESS_AUTOSCALE only: min / max / non-finite count over x with 16-byte loads; the block that takes the last ticket publishes them in words
//            [2], [3] and the (slope, inter) of egress_autoscale() below in words [6], [7].
//   convert  one block per 64 x 64 tile of the plane (file axis 0, file axis u) of one slab along the third file axis w.  Tiles are cut in FILE coordinates
//            along axis 0, so a thread always owns G = 16 / sizeof(output) consecutive file voxels and a reversed axis costs a register reversal, not a
//            narrower store: one 16-byte store wherever the group is whole and its address allows it (element-wise otherwise).
//              perm[2] == 0   x's fastest axis is file axis 0: straight from registers, u = file axis 1; 16- (or 8-) byte loads of the G source values
//              otherwise      u = perm[2], the file axis fed by x's fastest axis: every thread loads 16 bytes along x's fastest axis, the tile goes
//                             through LDS as tile[axis 0][u] with rows of 65 words and is read back with lanes along axis 0.  Per 32-lane half the reads
//                             cover 32 / G groups x G columns, words (G i + e) * 65 + j: banks (G i + e + j) mod 32, all distinct.
//            Without AUTOSCALE this launch also reduces min / max / count and publishes them (float32: the only launch).
// Min / max: order-free atomicMax on the order-preserving unsigned image of the float, as ingest.hip; the workspace must be ZERO when first used and
// then resets itself (words [0], [1], [4], [5]); words [2], [3], [6], [7] hold the last call's results.
#include "sa_common.h"

namespace sa {

enum { EG_F32 = 0, EG_I16 = 1, EG_U8 = 2 };

struct EgressGeom {
    int n0, n1, n2;          // file dims
    int ku;                  // file axis of the tile's second dimension (1 or 2); the slab axis is 3 - ku
    int nu, nw;
    uint32_t tiles0, tilesU, nblocks;
    int flip[3];             // per FILE axis k
    int64_t xstride[3];      // stride in x (elements) of the canonical axis that feeds file axis k
    int reduce, autoscale;
    double slope, inter;
};

__device__ __forceinline__ uint32_t egress_image(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float egress_value(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// THE auto-scaling rule (tests/nifti_out_ref.py: autoscale_ref): [mn, mx] covered by the code range [tmin, tmax], both numbers float32 because the header
// stores them as float32 and a reader applies the rounded ones.  A constant or empty volume: slope 1, inter = mn.
__device__ __forceinline__ void egress_autoscale(float mn, float mx, double tmin, double tmax, double* slope, double* inter) {
    if (!(mx > mn)) {
        *slope = 1.0;
        *inter = (double)mn;
        return;
    }
    const double range = tmax - tmin, span = (double)mx - (double)mn;
    float s = (float)(span / range);
    if ((double)s * range < span) s = __uint_as_float(__float_as_uint(s) + 1u);      // the next float32: the rounded slope must still cover the span
    *slope = (double)s;
    *inter = (double)(float)((double)mn - tmin * (double)s);
}

template <int OUT> __device__ __forceinline__ double egress_tmin() { return OUT == EG_I16 ? -32768.0 : 0.0; }
template <int OUT> __device__ __forceinline__ double egress_tmax() { return OUT == EG_I16 ? 32767.0 : 255.0; }

// the stored code of a FINITE value, in the low bits of a word
template <int OUT> __device__ __forceinline__ uint32_t egress_code(float v, double slope, double inter) {
    if (OUT == EG_F32) return __float_as_uint(v);
    double q = (double)v - inter;      // (two rounded operations: the build has -ffp-contract=off)
    q = q / slope;
    q = fmin(fmax(rint(q), egress_tmin<OUT>()), egress_tmax<OUT>());
    if (OUT == EG_I16) return (uint32_t)(uint16_t)(int16_t)(int)q;
    return (uint32_t)(uint8_t)(int)q;
}

template <int OUT> __device__ __forceinline__ void egress_store_one(unsigned char* raw, int64_t f, uint32_t code) {
    if (OUT == EG_F32) reinterpret_cast<uint32_t*>(raw)[f] = code;
    else if (OUT == EG_I16) reinterpret_cast<uint16_t*>(raw)[f] = (uint16_t)code;
    else raw[f] = (unsigned char)code;
}

// G codes -> four words
template <int OUT, int G> __device__ __forceinline__ u32x4 egress_pack(const uint32_t (&c)[G]) {
    u32x4 w;
    if (OUT == EG_F32) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = c[k];
    } else if (OUT == EG_I16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = c[2 * k] | (c[2 * k + 1] << 16);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = c[4 * k] | (c[4 * k + 1] << 8) | (c[4 * k + 2] << 16) | (c[4 * k + 3] << 24);
    }
    return w;
}

template <bool BF16> __device__ __forceinline__ float egress_load_one(const void* x, int64_t off) {
    return BF16 ? bf16_to_f32(reinterpret_cast<const bf16_t*>(x)[off]) : reinterpret_cast<const float*>(x)[off];
}
// element e of a run of source values held in words
template <bool BF16> __device__ __forceinline__ float egress_word_value(const uint32_t* w, int e) {
    return BF16 ? __uint_as_float((e & 1) ? (w[e >> 1] & 0xffff0000u) : (w[e >> 1] << 16)) : __uint_as_float(w[e]);
}

struct EgressAcc {
    float lo, hi;
    uint32_t cnt;
};
// a non-finite value becomes 0 and is counted; a finite one takes part in min / max
__device__ __forceinline__ float egress_screen(float v, EgressAcc& a) {
    if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) {
        ++a.cnt;
        return 0.f;
    }
    a.lo = fminf(a.lo, v);
    a.hi = fmaxf(a.hi, v);
    return v;
}

// block reduction of (lo, hi, cnt), the atomics, the ticket; the last block publishes and resets.  mode 1: the pair is egress_autoscale's, else the caller's.
__device__ __forceinline__ void egress_publish(EgressAcc a, unsigned long long* ws, uint32_t nblocks, float* red_lo, float* red_hi, uint32_t* red_cnt, int mode,
                                               double tmin, double tmax, double slope, double inter) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.lo = fminf(a.lo, __shfl_xor(a.lo, o, 64));
        a.hi = fmaxf(a.hi, __shfl_xor(a.hi, o, 64));
        a.cnt += __shfl_xor(a.cnt, o, 64);
    }
    if ((tid & 63u) == 0) {
        red_lo[tid >> 6] = a.lo;
        red_hi[tid >> 6] = a.hi;
        red_cnt[tid >> 6] = a.cnt;
    }
    __syncthreads();
    if (tid == 0) {
        const float lo = fminf(fminf(red_lo[0], red_lo[1]), fminf(red_lo[2], red_lo[3]));
        const float hi = fmaxf(fmaxf(red_hi[0], red_hi[1]), fmaxf(red_hi[2], red_hi[3]));
        const uint32_t cnt = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3];
        if (lo <= hi) {      // (a block without a finite voxel holds +inf / -inf)
            atomicMax(ws + 0, (unsigned long long)(uint32_t)(~egress_image(lo)));
            atomicMax(ws + 1, (unsigned long long)egress_image(hi));
        }
        if (cnt) atomicAdd(ws + 4, (unsigned long long)cnt);
        __threadfence();
        const unsigned long long ticket = atomicAdd(ws + 5, 1ull);
        if (ticket == (unsigned long long)nblocks - 1ull) {      // every other block's words are in: publish, and leave the workspace as it was found
            __threadfence();
            const unsigned long long klo = atomicExch(ws + 0, 0ull), khi = atomicExch(ws + 1, 0ull), bad = atomicExch(ws + 4, 0ull);
            atomicExch(ws + 5, 0ull);
            float mn = 0.f, mx = 0.f;
            if (khi != 0ull) {
                mn = egress_value(~(uint32_t)klo);
                mx = egress_value((uint32_t)khi);
            }
            ws[2] = (unsigned long long)__float_as_uint(mn) | ((unsigned long long)__float_as_uint(mx) << 32);
            ws[3] = bad;
            if (mode == 1) egress_autoscale(mn, mx, tmin, tmax, &slope, &inter);
            ws[6] = (unsigned long long)__double_as_longlong(slope);
            ws[7] = (unsigned long long)__double_as_longlong(inter);
        }
    }
}

template <bool BF16>
__global__ void __launch_bounds__(256) egress_reduce_kernel(const void* __restrict__ x, unsigned long long* __restrict__ ws, int64_t n, double tmin, double tmax) {
    constexpr int E = BF16 ? 8 : 4;
    __shared__ float red_lo[4], red_hi[4];
    __shared__ uint32_t red_cnt[4];
    EgressAcc a{INFINITY, -INFINITY, 0u};
    const int64_t ngroups = (n + E - 1) / E;
    const bool aligned = (((uintptr_t)x) & 15u) == 0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (int64_t)gridDim.x * 256) {
        const int64_t e0 = q * E;
        if (aligned && e0 + E <= n) {
            const u32x4 w = *reinterpret_cast<const u32x4*>((const unsigned char*)x + e0 * (BF16 ? 2 : 4));
            const uint32_t ww[4] = {w[0], w[1], w[2], w[3]};
#pragma unroll
            for (int e = 0; e < E; ++e) egress_screen(egress_word_value<BF16>(ww, e), a);
        } else {
            for (int e = 0; e < E; ++e)
                if (e0 + e < n) egress_screen(egress_load_one<BF16>(x, e0 + e), a);
        }
    }
    egress_publish(a, ws, gridDim.x, red_lo, red_hi, red_cnt, 1, tmin, tmax, 1.0, 0.0);
}

template <int OUT, bool BF16, bool STRAIGHT>
__global__ void __launch_bounds__(256) egress_tile_kernel(const void* __restrict__ x, unsigned char* __restrict__ raw, unsigned long long* __restrict__ ws,
                                                          const EgressGeom g) {
    constexpr int S = OUT == EG_F32 ? 4 : OUT == EG_I16 ? 2 : 1;      // bytes per output voxel
    constexpr int G = 16 / S;                                         // output voxels per 16-byte store
    constexpr int GR = 64 / G;                                        // groups per tile row
    __shared__ float tile[STRAIGHT ? 1 : 64 * 65];
    __shared__ float red_lo[4], red_hi[4];
    __shared__ uint32_t red_cnt[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t bt = blockIdx.x % g.tiles0, rest = blockIdx.x / g.tiles0;
    const uint32_t bu = rest % g.tilesU, w = rest / g.tilesU;
    const int t0 = (int)bt * 64, u0 = (int)bu * 64;
    const int kw = 3 - g.ku;
    const int64_t xw = (int64_t)(g.flip[kw] ? g.nw - 1 - (int)w : (int)w) * g.xstride[kw];
    double slope = g.slope, inter = g.inter;
    if (OUT != EG_F32 && g.autoscale) {      // what the reduce launch left on the device
        slope = __longlong_as_double((long long)ws[6]);
        inter = __longlong_as_double((long long)ws[7]);
    }
    EgressAcc a{INFINITY, -INFINITY, 0u};
    if (STRAIGHT) {
        for (uint32_t ch = tid; ch < 64u * GR; ch += 256u) {
            const int r = (int)(ch / GR), i0 = t0 + (int)(ch % GR) * G, i1 = u0 + r;
            if (i1 >= g.nu || i0 >= g.n0) continue;
            const int nvalid = min(G, g.n0 - i0);
            const int64_t base = (int64_t)(g.flip[1] ? g.nu - 1 - i1 : i1) * g.xstride[1] + xw;
            const int64_t f = (int64_t)i0 + (int64_t)g.n0 * ((int64_t)i1 + (int64_t)g.n1 * (int64_t)w);
            float v[G];
            constexpr int NW = G * (BF16 ? 2 : 4) / 4;      // words of G source values
            const int64_t xlo = base + (g.flip[0] ? g.n0 - i0 - G : i0);
            const unsigned char* p = (const unsigned char*)x + xlo * (BF16 ? 2 : 4);
            if (nvalid == G && (((uintptr_t)p) & (NW >= 4 ? 15u : 7u)) == 0) {
                uint32_t ww[NW];
                if (NW >= 4) {
#pragma unroll
                    for (int k = 0; k < NW / 4; ++k) {
                        const u32x4 q = reinterpret_cast<const u32x4*>(p)[k];
                        ww[4 * k] = q[0]; ww[4 * k + 1] = q[1]; ww[4 * k + 2] = q[2]; ww[4 * k + 3] = q[3];
                    }
                } else {
                    const uint2 q = *reinterpret_cast<const uint2*>(p);
                    ww[0] = q.x; ww[1] = q.y;
                }
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    const float fwd = egress_word_value<BF16>(ww, e), rev = egress_word_value<BF16>(ww, G - 1 - e);
                    v[e] = g.flip[0] ? rev : fwd;
                }
            } else {
#pragma unroll
                for (int e = 0; e < G; ++e) v[e] = e < nvalid ? egress_load_one<BF16>(x, base + (g.flip[0] ? g.n0 - 1 - (i0 + e) : i0 + e)) : 0.f;
            }
            uint32_t code[G];
#pragma unroll
            for (int e = 0; e < G; ++e) {
                if (e < nvalid) v[e] = egress_screen(v[e], a);
                code[e] = egress_code<OUT>(v[e], slope, inter);
            }
            unsigned char* o = raw + f * S;
            if (nvalid == G && (((uintptr_t)o) & 15u) == 0) {
                *reinterpret_cast<u32x4*>(o) = egress_pack<OUT, G>(code);
            } else {
#pragma unroll
                for (int e = 0; e < G; ++e)
                    if (e < nvalid) egress_store_one<OUT>(raw, f + e, code[e]);
            }
        }
    } else {
        constexpr int E = BF16 ? 8 : 4;      // source values per 16-byte load
        constexpr int CR = 64 / E;
        // rows: file axis 0 (i0 = t0 + r); columns: x's fastest axis (xc = u0 + c), which is file axis ku read forwards or backwards
        for (uint32_t ch = tid; ch < 64u * CR; ch += 256u) {
            const int r = (int)(ch / CR), c = (int)(ch % CR) * E;
            const int i0 = t0 + r, xc = u0 + c;
            if (i0 >= g.n0 || xc >= g.nu) continue;
            const int nvalid = min(E, g.nu - xc);
            const int64_t off = (int64_t)(g.flip[0] ? g.n0 - 1 - i0 : i0) * g.xstride[0] + xw + xc;
            const unsigned char* p = (const unsigned char*)x + off * (BF16 ? 2 : 4);
            float v[E];
            if (nvalid == E && (((uintptr_t)p) & 15u) == 0) {
                const u32x4 q = *reinterpret_cast<const u32x4*>(p);
                const uint32_t ww[4] = {q[0], q[1], q[2], q[3]};
#pragma unroll
                for (int e = 0; e < E; ++e) v[e] = egress_word_value<BF16>(ww, e);
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) v[e] = e < nvalid ? egress_load_one<BF16>(x, off + e) : 0.f;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e < nvalid) v[e] = egress_screen(v[e], a);
                tile[r * 65 + c + e] = v[e];
            }
        }
        __syncthreads();
        constexpr int IL = 32 / G;      // lanes along axis 0 per 32-lane half
        for (uint32_t it = tid; it < 64u * GR; it += 256u) {
            const int lane = (int)(it & 63u), li = lane & 31;
            const int i = (li % IL) + IL * (lane >> 5), j = (int)(it >> 6) * G + li / IL;
            const int i0 = t0 + i * G, xc = u0 + j;
            if (i0 >= g.n0 || xc >= g.nu) continue;
            const int nvalid = min(G, g.n0 - i0);
            const int iu = g.flip[g.ku] ? g.nu - 1 - xc : xc;
            const int i1 = g.ku == 1 ? iu : (int)w, i2 = g.ku == 1 ? (int)w : iu;
            const int64_t f = (int64_t)i0 + (int64_t)g.n0 * ((int64_t)i1 + (int64_t)g.n1 * i2);
            uint32_t code[G];
#pragma unroll
            for (int e = 0; e < G; ++e) code[e] = egress_code<OUT>(tile[(i * G + e) * 65 + j], slope, inter);      // (rows past n0 were never written: not stored)
            unsigned char* o = raw + f * S;
            if (nvalid == G && (((uintptr_t)o) & 15u) == 0) {
                *reinterpret_cast<u32x4*>(o) = egress_pack<OUT, G>(code);
            } else {
#pragma unroll
                for (int e = 0; e < G; ++e)
                    if (e < nvalid) egress_store_one<OUT>(raw, f + e, code[e]);
            }
        }
    }
    if (g.reduce) egress_publish(a, ws, g.nblocks, red_lo, red_hi, red_cnt, 0, 0.0, 0.0, slope, inter);
}

template <int OUT, bool BF16> static int egress_launch(const void* x, unsigned char* raw, unsigned long long* ws, const EgressGeom& g, bool straight, hipStream_t stream) {
    if (straight) SA_LAUNCH((egress_tile_kernel<OUT, BF16, true>), dim3(g.nblocks), dim3(256), 0, stream, x, raw, ws, g);
    else SA_LAUNCH((egress_tile_kernel<OUT, BF16, false>), dim3(g.nblocks), dim3(256), 0, stream, x, raw, ws, g);
    SA_CHECK_LAUNCH();
    return 0;
}
template <int OUT> static int egress_launch_in(const void* x, bool bf16, unsigned char* raw, unsigned long long* ws, const EgressGeom& g, bool straight, hipStream_t stream) {
    return bf16 ? egress_launch<OUT, true>(x, raw, ws, g, straight, stream) : egress_launch<OUT, false>(x, raw, ws, g, straight, stream);
}

}  // namespace sa

using namespace sa;

extern "C" int64_t sa_volume_egress_workspace_bytes(void) { return 64; }

extern "C" int sa_volume_egress(const void* x, void* raw, int64_t raw_bytes, const sa_egress_params* params, void* ws, void* stream) {
    if (!x || !raw || !params || !ws || (((uintptr_t)raw) & 15u) != 0 || (((uintptr_t)ws) & 7u) != 0) return SA_EINVAL;
    const sa_egress_params& P = *params;
    for (int a = 0; a < 3; ++a)
        if (P.ext[a] < 1) return SA_EINVAL;
    const int p0 = P.perm[0], p1 = P.perm[1], p2 = P.perm[2];
    if (p0 < 0 || p0 > 2 || p1 < 0 || p1 > 2 || p2 < 0 || p2 > 2 || p0 == p1 || p0 == p2 || p1 == p2) return SA_EINVAL;
    if (P.x_dtype != SA_F32 && P.x_dtype != SA_BF16) return SA_EUNSUPPORTED;
    int size;
    switch (P.dtype) {
        case SA_NII_FLOAT32: size = 4; break;
        case SA_NII_INT16: size = 2; break;
        case SA_NII_UINT8: size = 1; break;
        default: return SA_EUNSUPPORTED;
    }
    const int64_t plane = (int64_t)P.ext[0] * P.ext[1];      // < 2^62
    if (plane > 0x7ffffff0ll || plane * P.ext[2] >= 0x7ffffff0ll) return SA_EUNSUPPORTED;
    const int64_t nvox = plane * P.ext[2];
    if (raw_bytes < nvox * size) return SA_EINVAL;
    const bool integer = P.dtype != SA_NII_FLOAT32, autoscale = integer && (P.flags & SA_EGRESS_AUTOSCALE) != 0;
    if (integer && !autoscale && !(P.slope != 0.0 && P.slope - P.slope == 0.0 && P.inter - P.inter == 0.0)) return SA_EINVAL;      // a zero or non-finite pair
    EgressGeom g;
    int n[3];
    const int64_t xs[3] = {(int64_t)P.ext[1] * P.ext[2], (int64_t)P.ext[2], 1};
    for (int a = 0; a < 3; ++a) {
        const int k = P.perm[a];
        n[k] = P.ext[a];
        g.flip[k] = P.sign[a] < 0;
        g.xstride[k] = xs[a];
    }
    g.n0 = n[0]; g.n1 = n[1]; g.n2 = n[2];
    const bool straight = p2 == 0;
    g.ku = straight ? 1 : p2;
    g.nu = n[g.ku];
    g.nw = n[3 - g.ku];
    g.tiles0 = (uint32_t)((g.n0 + 63) / 64);
    g.tilesU = (uint32_t)((g.nu + 63) / 64);
    g.nblocks = g.tiles0 * g.tilesU * (uint32_t)g.nw;      // <= nvox
    g.reduce = !autoscale;
    g.autoscale = autoscale;
    g.slope = integer ? P.slope : 1.0;
    g.inter = integer ? P.inter : 0.0;
    unsigned long long* w = (unsigned long long*)ws;
    const bool bf16 = P.x_dtype == SA_BF16;
    if (autoscale) {
        const int64_t ngroups = (nvox + (bf16 ? 8 : 4) - 1) / (bf16 ? 8 : 4);
        const unsigned blocks = (unsigned)((ngroups + 255) / 256 < 2048 ? (ngroups + 255) / 256 : 2048);
        const double tmin = P.dtype == SA_NII_INT16 ? -32768.0 : 0.0, tmax = P.dtype == SA_NII_INT16 ? 32767.0 : 255.0;
        if (bf16) SA_LAUNCH((egress_reduce_kernel<true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, w, nvox, tmin, tmax);
        else SA_LAUNCH((egress_reduce_kernel<false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, w, nvox, tmin, tmax);
        SA_CHECK_LAUNCH();
    }
    unsigned char* r = (unsigned char*)raw;
    return P.dtype == SA_NII_FLOAT32 ? egress_launch_in<EG_F32>(x, bf16, r, w, g, straight, (hipStream_t)stream)
         : P.dtype == SA_NII_INT16   ? egress_launch_in<EG_I16>(x, bf16, r, w, g, straight, (hipStream_t)stream)
                                     : egress_launch_in<EG_U8>(x, bf16, r, w, g, straight, (hipStream_t)stream);
}
