// The per-volume summary record of an anomaly map (SA_ANOMALY_RESULT_WORDS words, include/synthanatomy_hip.h: sa_anomaly_map), shared by
// csrc/anomaly.hip (sa_anomaly_map, sa_anomaly_map_ensemble) and csrc/median.hip (sa_anomaly_median) so that both fill it by the same code.
// A block of AN_THREADS = 256 threads (four waves) that never straddles volumes
//   - counts every voxel it owns with an_account() (registers, and LDS atomics for the histogram bins above 0),
//   - leaves AN_PART 64-bit words in the workspace with an_block_finish(): sum a as fp64, max a, bin 0 of class 0 and of class 1, TP, FP, FN,
//     and adds its other bins to the record with 64-bit integer atomics;
// one block per volume then adds the partial words in a fixed order (an_finish_body()): no float atomics, the same bits alone or in any batch.
#pragma once
#include "sa_common.h"

namespace sa {

constexpr int AN_THREADS = 256;
constexpr int AN_WORDS = SA_ANOMALY_RESULT_WORDS;
constexpr int AN_PART = 8;                           // 64-bit words a block leaves in the workspace
constexpr int AN_TAIL_BYTES = 512 * 4 + 4 * 8 + 4 * 4 + 20 * 4;      // LDS of a block's summary: the 2 x 256 histogram, per wave one fp64, one fp32, five counts

__device__ __forceinline__ double an_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float an_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t an_wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a thread's running summary: cnt = bin 0 of class 0, bin 0 of class 1, TP, FP, FN
struct AnAcc {
    double bs = 0.0;
    float bm = 0.f;
    uint32_t cnt[5] = {0u, 0u, 0u, 0u, 0u};
};

// a block's summary buffers inside `tail` (AN_TAIL_BYTES bytes of LDS, 8-byte aligned); hist must be cleared and a barrier passed before an_account()
struct AnTail {
    uint32_t* hist;      // [2][256]
    double* red_s;       // [4]
    float* red_m;        // [4]
    uint32_t* red_c;     // [5][4]
};
__device__ __forceinline__ AnTail an_tail(char* tail) {
    return AnTail{reinterpret_cast<uint32_t*>(tail), reinterpret_cast<double*>(tail + 512 * 4), reinterpret_cast<float*>(tail + 512 * 4 + 4 * 8),
                  reinterpret_cast<uint32_t*>(tail + 512 * 4 + 4 * 8 + 4 * 4)};
}

// one voxel: value a, label class cls (0 / 1).  bin = min(255, (int)(a * inv_bin)), the product one fp32 multiply; a product below zero counts in bin 0
// (sa_anomaly_map's values are never negative), a NaN in bin 255.
__device__ __forceinline__ void an_account(AnAcc& A, uint32_t* hist, float a, uint32_t cls, float inv_bin, bool has_t, float t) {
    A.bs += (double)a;
    A.bm = fmaxf(A.bm, a);
    float scaled = a * inv_bin;
    scaled = scaled < 0.f ? 0.f : scaled;
    const int bin = (int)fminf(scaled, 255.f);
    if (bin == 0) {
        A.cnt[0] += cls ^ 1u;
        A.cnt[1] += cls;
    } else {
        atomicAdd(&hist[cls * 256u + (uint32_t)bin], 1u);
    }
    if (has_t) {
        const uint32_t pred = a >= t ? 1u : 0u;
        A.cnt[2] += pred & cls;
        A.cnt[3] += pred & (cls ^ 1u);
        A.cnt[4] += (pred ^ 1u) & cls;
    }
}

// every thread of the block calls this once, after its last an_account(): pp = the block's AN_PART words, res = the volume's record
__device__ __forceinline__ void an_block_finish(AnAcc& A, const AnTail& T, unsigned long long* __restrict__ pp, unsigned long long* __restrict__ res) {
    const int tid = threadIdx.x;
    double bs = an_wave_sum_f64(A.bs);
    float bm = an_wave_max(A.bm);
    uint32_t cnt[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) cnt[q] = an_wave_sum_u32(A.cnt[q]);
    if ((tid & 63) == 0) {
        T.red_s[tid >> 6] = bs;
        T.red_m[tid >> 6] = bm;
#pragma unroll
        for (int q = 0; q < 5; ++q) T.red_c[q * 4 + (tid >> 6)] = cnt[q];
    }
    __syncthreads();
    if (tid == 0) {
        pp[0] = (unsigned long long)__double_as_longlong((T.red_s[0] + T.red_s[1]) + (T.red_s[2] + T.red_s[3]));
        pp[1] = (unsigned long long)__double_as_longlong((double)fmaxf(fmaxf(T.red_m[0], T.red_m[1]), fmaxf(T.red_m[2], T.red_m[3])));
    } else if (tid < 6) {
        const uint32_t* c = T.red_c + (tid - 1) * 4;
        pp[1 + tid] = (unsigned long long)c[0] + c[1] + c[2] + c[3];
    }
    for (int i = tid; i < 512; i += AN_THREADS) {      // (words 0 and 256 stay empty here: bin 0 travels through the workspace)
        const uint32_t v = T.hist[i];
        if (v) atomicAdd(res + 8 + i, (unsigned long long)v);
    }
}

// results[b][0] = sum a, [1] = max a (both as doubles), [2..4] = TP, FP, FN, [8] and [8 + 256] = bin 0 of the two classes: one block of 256 threads per
// volume (b = blockIdx.x), lanes and waves in a fixed order
__device__ __forceinline__ void an_finish_body(const unsigned long long* __restrict__ part, int nblk, unsigned long long* __restrict__ results) {
    __shared__ double red_s[4], red_m[4];
    __shared__ unsigned long long red_c[5][4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const unsigned long long* pp = part + b * nblk * AN_PART;
    double s = 0.0, mx = 0.0;
    unsigned long long c[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (int i = tid; i < nblk; i += 256) {
        s += __longlong_as_double((long long)pp[AN_PART * i]);
        mx = fmax(mx, __longlong_as_double((long long)pp[AN_PART * i + 1]));
#pragma unroll
        for (int q = 0; q < 5; ++q) c[q] += pp[AN_PART * i + 2 + q];
    }
    s = an_wave_sum_f64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, o, 64));
#pragma unroll
        for (int q = 0; q < 5; ++q) c[q] += __shfl_xor(c[q], o, 64);
    }
    if ((tid & 63) == 0) {
        red_s[tid >> 6] = s;
        red_m[tid >> 6] = mx;
#pragma unroll
        for (int q = 0; q < 5; ++q) red_c[q][tid >> 6] = c[q];
    }
    __syncthreads();
    unsigned long long* res = results + b * AN_WORDS;
    if (tid == 0) {
        res[0] = (unsigned long long)__double_as_longlong((red_s[0] + red_s[1]) + (red_s[2] + red_s[3]));
        res[1] = (unsigned long long)__double_as_longlong(fmax(fmax(red_m[0], red_m[1]), fmax(red_m[2], red_m[3])));
    } else if (tid < 6) {
        const int q = tid - 1;
        const unsigned long long v = red_c[q][0] + red_c[q][1] + red_c[q][2] + red_c[q][3];
        res[q == 0 ? 8 : q == 1 ? 8 + 256 : q] = v;      // q = 2, 3, 4: TP, FP, FN sit in words 2, 3, 4
    }
}

}  // namespace sa
