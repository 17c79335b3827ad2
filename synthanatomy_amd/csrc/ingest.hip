// NIfTI-1 voxel block -> fp32 volume in canonical axes, on the device: sa_volume_ingest (include/synthanatomy_hip.h).  What the reference does on
// the host with LoadImaged(as_closest_canonical) / AddChanneld / ScaleIntensityd(0, 1) / the ROI crop (reference src/utils/vqvae.py:205-215).
//
// The file is axis-0-fastest (offset i0 + n0 (i1 + n1 i2)), the output y[ext0][ext1][ext2] is last-axis-fastest, and canonical axis a reads file axis
// perm[a] (backwards where sign[a] < 0).  Two launches on the caller's stream, no host synchronisation:
//   pass 1  one block per 64 x 64 tile of the plane (file axis 0, file axis u) of one slab along the third file axis w.  Every thread reads 16-byte
//           chunks along file axis 0 (2 / 4 / 8 / 16 elements; element-wise where a row is not 16-byte aligned or the chunk crosses the row's end),
//           swaps bytes, widens to fp32 (through two rounded fp64 operations when the file carries a scale), replaces non-finite values by 0 and counts
//           them, and reduces min / max over EVERY voxel of the file.  Then the part of the tile that lies inside the window is written:
//             perm[2] == 0   file axis 0 is the output's fastest axis: straight from registers, u = file axis 1 (a coalesced copy, 16-byte stores where
//                            the row is not reversed and the address allows it)
//             otherwise      u = perm[2], the file axis that feeds the output's fastest axis: the tile goes through LDS as tile[u][axis 0] with rows of
//                            65 words, is read back column-wise (lane = u: word stride 65 = 1 mod 64 banks, conflict-free) and written with lanes along
//                            the output's fastest axis.  The row-wise LDS writes of pass 1 are conflict-free with the same padding: the lanes of a wave
//                            cover 64 / CR rows of CR chunks each, banks (row + E * chunk + e) mod 64, all distinct.
//   pass 2  SA_INGEST_NORMALIZE only: y = (v - min) / ((max - min) + 1e-8f) in place over the window.
// Min / max: order-free atomicMax on the order-preserving unsigned image of the float (inverted for the minimum), as the gamma step of augment.hip; 0 is
// below the key of every finite float, so the cleared workspace is the identity.  The block that takes the last ticket publishes min / max and the
// non-finite count in words [2], [3] and puts the reduction words back to 0: the workspace must be ZERO when first used and then resets itself.
#include "sa_common.h"

namespace sa {

enum { ING_UINT = 0, ING_SINT = 1, ING_FLOAT = 2 };

struct IngestGeom {
    int n0, n1, n2;          // file dims
    int ku;                  // file axis of the tile's second dimension (1 or 2); the slab axis is 3 - ku
    int nu, nw;
    uint32_t tiles0, tilesU, nblocks;
    int kind, swap, scaled;
    double slope, inter;
    // per FILE axis k (feeding canonical axis a): output coordinate o = flip ? base - i : i - base, inside the window when 0 <= o < ext
    int flip[3], base[3], ext[3];
    int64_t ystride[3];
    int64_t nout;
};

__device__ __forceinline__ uint32_t ingest_image(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ingest_value(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// element e of a 16-byte chunk held in four registers
template <int S> __device__ __forceinline__ uint64_t chunk_bits(const u32x4& w, int e) {
    if (S == 1) return (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
    if (S == 2) return (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    if (S == 4) return w[e];
    return (uint64_t)w[2 * e] | ((uint64_t)w[2 * e + 1] << 32);
}
template <int S> __device__ __forceinline__ uint64_t load_bits(const unsigned char* p) {
    if (S == 1) return *p;
    if (S == 2) return *reinterpret_cast<const uint16_t*>(p);
    if (S == 4) return *reinterpret_cast<const uint32_t*>(p);
    return *reinterpret_cast<const uint64_t*>(p);
}

template <int S> __device__ __forceinline__ float ingest_convert(uint64_t bits, const IngestGeom& g) {
    if (g.swap) {
        if (S == 2) bits = __builtin_bswap16((uint16_t)bits);
        if (S == 4) bits = __builtin_bswap32((uint32_t)bits);
        if (S == 8) bits = __builtin_bswap64(bits);
    }
    if (!g.scaled) {
        if (S == 8) return (float)__longlong_as_double((long long)bits);
        if (S == 4) return g.kind == ING_FLOAT ? __uint_as_float((uint32_t)bits) : g.kind == ING_SINT ? (float)(int32_t)(uint32_t)bits : (float)(uint32_t)bits;
        if (S == 2) return g.kind == ING_SINT ? (float)(int16_t)(uint16_t)bits : (float)(uint16_t)bits;
        return g.kind == ING_SINT ? (float)(int8_t)(uint8_t)bits : (float)(uint8_t)bits;
    }
    double d;
    if (S == 8) d = __longlong_as_double((long long)bits);
    else if (S == 4) d = g.kind == ING_FLOAT ? (double)__uint_as_float((uint32_t)bits) : g.kind == ING_SINT ? (double)(int32_t)(uint32_t)bits : (double)(uint32_t)bits;
    else if (S == 2) d = g.kind == ING_SINT ? (double)(int16_t)(uint16_t)bits : (double)(uint16_t)bits;
    else d = g.kind == ING_SINT ? (double)(int8_t)(uint8_t)bits : (double)(uint8_t)bits;
    d = d * g.slope;      // (two rounded operations: the build has -ffp-contract=off)
    d = d + g.inter;
    return (float)d;
}

template <int S, bool STRAIGHT>
__global__ void __launch_bounds__(256) ingest_tile_kernel(const unsigned char* __restrict__ raw, float* __restrict__ y, unsigned long long* __restrict__ ws,
                                                          const IngestGeom g) {
    constexpr int E = 16 / S;           // elements per 16-byte chunk
    constexpr int CR = 64 / E;          // chunks per tile row
    __shared__ float tile[STRAIGHT ? 1 : 64 * 65];
    __shared__ float red_lo[4], red_hi[4];
    __shared__ uint32_t red_cnt[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t bt = blockIdx.x % g.tiles0, rest = blockIdx.x / g.tiles0;
    const uint32_t bu = rest % g.tilesU, w = rest / g.tilesU;
    const int t0 = (int)bt * 64, u0 = (int)bu * 64;
    const int kw = 3 - g.ku;
    const int ow = g.flip[kw] ? g.base[kw] - (int)w : (int)w - g.base[kw];
    const bool slab_in = ow >= 0 && ow < g.ext[kw];
    float lo = INFINITY, hi = -INFINITY;
    uint32_t cnt = 0;
    for (uint32_t ch = tid; ch < 64u * CR; ch += 256u) {
        const int r = (int)(ch / CR), c0 = (int)(ch % CR) * E;
        const int iu = u0 + r, i0 = t0 + c0;
        if (iu >= g.nu || i0 >= g.n0) continue;
        const int i1 = g.ku == 1 ? iu : (int)w, i2 = g.ku == 1 ? (int)w : iu;
        const int64_t f = (int64_t)i0 + (int64_t)g.n0 * ((int64_t)i1 + (int64_t)g.n1 * i2);
        const unsigned char* p = raw + f * S;
        const int nvalid = min(E, g.n0 - i0);
        float v[E];
        if (nvalid == E && (((uintptr_t)p) & 15u) == 0) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = ingest_convert<S>(chunk_bits<S>(q, e), g);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = e < nvalid ? ingest_convert<S>(load_bits<S>(p + e * S), g) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (e < nvalid) {
                if ((__float_as_uint(v[e]) & 0x7f800000u) == 0x7f800000u) {
                    v[e] = 0.f;
                    ++cnt;
                } else {
                    lo = fminf(lo, v[e]);
                    hi = fmaxf(hi, v[e]);
                }
            }
        }
        if (STRAIGHT) {
            const int ou = g.flip[1] ? g.base[1] - iu : iu - g.base[1];
            if (slab_in && ou >= 0 && ou < g.ext[1]) {
                float* yp = y + (int64_t)ou * g.ystride[1] + (int64_t)ow * g.ystride[2];
                const int o0 = i0 - g.base[0];
                if (E >= 4 && !g.flip[0] && nvalid == E && o0 >= 0 && o0 + E <= g.ext[0] && (((uintptr_t)(yp + o0)) & 15u) == 0) {
#pragma unroll
                    for (int e = 0; e + 3 < E; e += 4) *reinterpret_cast<float4_t*>(yp + o0 + e) = float4_t{v[e], v[e + 1], v[e + 2], v[e + 3]};
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const int o = g.flip[0] ? g.base[0] - (i0 + e) : (i0 + e) - g.base[0];
                        if (e < nvalid && o >= 0 && o < g.ext[0]) yp[o] = v[e];
                    }
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) tile[r * 65 + c0 + e] = v[e];
        }
    }
    if (!STRAIGHT) {
        __syncthreads();
        if (slab_in) {
            const int r = (int)(tid & 63u), iu = u0 + r;
            const int ou = g.flip[g.ku] ? g.base[g.ku] - iu : iu - g.base[g.ku];
            if (iu < g.nu && ou >= 0 && ou < g.ext[g.ku]) {
                float* yp = y + (int64_t)ou * g.ystride[g.ku] + (int64_t)ow * g.ystride[kw];
                for (int c = (int)(tid >> 6); c < 64; c += 4) {
                    const int i0 = t0 + c;
                    const int o0 = g.flip[0] ? g.base[0] - i0 : i0 - g.base[0];
                    if (i0 < g.n0 && o0 >= 0 && o0 < g.ext[0]) yp[(int64_t)o0 * g.ystride[0]] = tile[r * 65 + c];
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((tid & 63u) == 0) {
        red_lo[tid >> 6] = lo;
        red_hi[tid >> 6] = hi;
        red_cnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        lo = fminf(fminf(red_lo[0], red_lo[1]), fminf(red_lo[2], red_lo[3]));
        hi = fmaxf(fmaxf(red_hi[0], red_hi[1]), fmaxf(red_hi[2], red_hi[3]));
        cnt = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3];
        if (lo <= hi) {      // (a block without a finite voxel holds +inf / -inf)
            atomicMax(ws + 0, (unsigned long long)(uint32_t)(~ingest_image(lo)));
            atomicMax(ws + 1, (unsigned long long)ingest_image(hi));
        }
        if (cnt) atomicAdd(ws + 4, (unsigned long long)cnt);
        __threadfence();
        const unsigned long long ticket = atomicAdd(ws + 5, 1ull);
        if (ticket == (unsigned long long)g.nblocks - 1ull) {      // every other block's words are in: publish, and leave the workspace as it was found
            __threadfence();
            const unsigned long long klo = atomicExch(ws + 0, 0ull), khi = atomicExch(ws + 1, 0ull), bad = atomicExch(ws + 4, 0ull);
            atomicExch(ws + 5, 0ull);
            float mn = 0.f, mx = 0.f;
            if (khi != 0ull) {
                mn = ingest_value(~(uint32_t)klo);
                mx = ingest_value((uint32_t)khi);
            }
            ws[2] = (unsigned long long)__float_as_uint(mn) | ((unsigned long long)__float_as_uint(mx) << 32);
            ws[3] = bad;
        }
    }
}

__global__ void __launch_bounds__(256) ingest_normalize_kernel(float* __restrict__ y, const unsigned long long* __restrict__ ws, int64_t nout) {
    const unsigned long long mm = ws[2];
    const float mn = __uint_as_float((uint32_t)mm), mx = __uint_as_float((uint32_t)(mm >> 32));
    const float den = (mx - mn) + 1e-8f;
    const int64_t ngroups = (nout + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (int64_t)gridDim.x * 256) {
        float* p = y + q * 4;
        if (q * 4 + 3 < nout && (((uintptr_t)p) & 15u) == 0) {
            float4_t t = *reinterpret_cast<const float4_t*>(p);
            t.x = (t.x - mn) / den; t.y = (t.y - mn) / den; t.z = (t.z - mn) / den; t.w = (t.w - mn) / den;
            *reinterpret_cast<float4_t*>(p) = t;
        } else {
            for (int r = 0; r < 4; ++r)
                if (q * 4 + r < nout) p[r] = (p[r] - mn) / den;
        }
    }
}

template <int S> static int ingest_launch(const unsigned char* raw, float* y, unsigned long long* ws, const IngestGeom& g, bool straight, hipStream_t stream) {
    if (straight) SA_LAUNCH((ingest_tile_kernel<S, true>), dim3(g.nblocks), dim3(256), 0, stream, raw, y, ws, g);
    else SA_LAUNCH((ingest_tile_kernel<S, false>), dim3(g.nblocks), dim3(256), 0, stream, raw, y, ws, g);
    SA_CHECK_LAUNCH();
    return 0;
}

}  // namespace sa

using namespace sa;

extern "C" int64_t sa_volume_ingest_workspace_bytes(void) { return 64; }

extern "C" int sa_volume_ingest(const void* raw, int64_t raw_bytes, float* y, const sa_ingest_params* params, void* ws, void* stream) {
    if (!raw || !y || !params || !ws || (((uintptr_t)raw) & 15u) != 0 || (((uintptr_t)ws) & 7u) != 0) return SA_EINVAL;
    const sa_ingest_params& P = *params;
    for (int a = 0; a < 3; ++a)
        if (P.n[a] < 1 || P.ext[a] < 1) return SA_EINVAL;
    const int p0 = P.perm[0], p1 = P.perm[1], p2 = P.perm[2];
    if (p0 < 0 || p0 > 2 || p1 < 0 || p1 > 2 || p2 < 0 || p2 > 2 || p0 == p1 || p0 == p2 || p1 == p2) return SA_EINVAL;
    for (int a = 0; a < 3; ++a)
        if (P.off[a] < 0 || (int64_t)P.off[a] + P.ext[a] > P.n[P.perm[a]]) return SA_EINVAL;
    int size, kind;
    switch (P.dtype) {
        case SA_NII_UINT8: size = 1; kind = ING_UINT; break;
        case SA_NII_INT8: size = 1; kind = ING_SINT; break;
        case SA_NII_INT16: size = 2; kind = ING_SINT; break;
        case SA_NII_UINT16: size = 2; kind = ING_UINT; break;
        case SA_NII_INT32: size = 4; kind = ING_SINT; break;
        case SA_NII_UINT32: size = 4; kind = ING_UINT; break;
        case SA_NII_FLOAT32: size = 4; kind = ING_FLOAT; break;
        case SA_NII_FLOAT64: size = 8; kind = ING_FLOAT; break;
        default: return SA_EUNSUPPORTED;
    }
    const int64_t plane = (int64_t)P.n[0] * P.n[1];      // < 2^62
    if (plane > 0x7ffffff0ll || plane * P.n[2] >= 0x7ffffff0ll) return SA_EUNSUPPORTED;
    const int64_t nvox = plane * P.n[2];
    if (raw_bytes < nvox * size) return SA_EINVAL;
    IngestGeom g;
    g.n0 = P.n[0]; g.n1 = P.n[1]; g.n2 = P.n[2];
    const bool straight = p2 == 0;
    g.ku = straight ? 1 : p2;
    g.nu = P.n[g.ku];
    g.nw = P.n[3 - g.ku];
    g.tiles0 = (uint32_t)((g.n0 + 63) / 64);
    g.tilesU = (uint32_t)((g.nu + 63) / 64);
    g.nblocks = g.tiles0 * g.tilesU * (uint32_t)g.nw;      // <= nvox
    g.kind = kind;
    g.swap = P.byteswap != 0 && size > 1;
    g.scaled = !(P.slope == 1.0 && P.inter == 0.0);
    g.slope = P.slope;
    g.inter = P.inter;
    const int64_t ys[3] = {(int64_t)P.ext[1] * P.ext[2], (int64_t)P.ext[2], 1};
    for (int a = 0; a < 3; ++a) {
        const int k = P.perm[a];
        g.flip[k] = P.sign[a] < 0;
        g.base[k] = g.flip[k] ? P.n[k] - 1 - P.off[a] : P.off[a];
        g.ext[k] = P.ext[a];
        g.ystride[k] = ys[a];
    }
    g.nout = (int64_t)P.ext[0] * P.ext[1] * P.ext[2];
    const unsigned char* r = (const unsigned char*)raw;
    unsigned long long* w = (unsigned long long*)ws;
    int rc = size == 1 ? ingest_launch<1>(r, y, w, g, straight, (hipStream_t)stream)
           : size == 2 ? ingest_launch<2>(r, y, w, g, straight, (hipStream_t)stream)
           : size == 4 ? ingest_launch<4>(r, y, w, g, straight, (hipStream_t)stream)
                       : ingest_launch<8>(r, y, w, g, straight, (hipStream_t)stream);
    if (rc != 0) return rc;
    if (P.flags & SA_INGEST_NORMALIZE) {
        const int64_t ngroups = (g.nout + 3) >> 2;
        const unsigned blocks = (unsigned)((ngroups + 255) / 256 < 65536 ? (ngroups + 255) / 256 : 65536);
        SA_LAUNCH(ingest_normalize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, y, (const unsigned long long*)w, g.nout);
        SA_CHECK_LAUNCH();
    }
    return 0;
}
