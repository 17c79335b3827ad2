// Voxel-space anomaly map of a healed volume: sa_anomaly_map (include/synthanatomy_hip.h).  Per volume, with x the scan, r the decoded
// healed codes and m an optional latent weight grid (the resampling mask or the NLL map of Performer.heal) on a grid f_D x f_H x f_W times coarser:
//   e = |x - r|, max(x - r, 0) or max(r - x, 0);   u = m upsampled by nearest cell, zero outside the volume;
//   w = u filtered with the separable (2R + 1)-tap Gaussian g ("same" size);   a = e w   (a = e without a weight grid)
// and the summaries sum a, max a, a 256-bin histogram of a per label class and TP / FP / FN of [a >= t] against the label.
//
// One way to filter.  u is piecewise constant, so the filter along one axis is a banded operator from latent cells to voxels:
//   A[p][c] = sum of the taps g[t], |t| <= R, whose voxel p + t lies in cell c (c f <= p + t < (c + 1) f),   w = A_D A_H A_W m.
// A row has at most 2 ceil(R / f) + 1 entries that are not zero, and zero padding needs no code: a tap that leaves the volume lies in no cell.  A block
// owns a tile of 8 x 32 (H x W) voxels and a run of 16 planes along D, one (h, w) column per thread.  It builds the three band tables for its tile in LDS
// (entry = its taps added in ascending order), then walks the latent planes c_D its run can see: the plane's (cells_H x cells_W) neighbourhood goes
// through LDS, A_W is applied for the tile's 32 columns, every thread applies its row of A_H, and the value is folded into the thread's 16 plane
// accumulators with A_D.  Neither u nor w ever exists in memory; per voxel the kernel reads x, r and one optional label byte and writes a.
// The x / r / label loads of all 16 planes are issued before the filter, which hides their latency.
//
// Summaries: every block leaves eight 64-bit words in the workspace -- sum a as fp64, max a, its bin-0 voxels of class 0 and of class 1, TP, FP, FN -- and
// one block per volume adds them in a fixed order: no float atomics, and since a block never straddles volumes and the tiling depends on the volume's
// shape only, a volume's map and summaries are bitwise the same alone or in any batch.  The counts every block contributes to (bin 0 of both classes:
// most of a masked map is zero; TP / FP / FN) go that way too, counted in registers: thousands of blocks adding to ONE address serialise in L2 (measured:
// 420 us instead of 75 for a 160 x 224 x 160 volume).  The other bins are LDS atomics per block, then 64-bit global atomic adds of the bins that are not
// empty, 512 contiguous bytes per wave instruction.
//
// Ensembles: sa_anomaly_map_ensemble is the same body with a loop over K members (r_k, m_k) inside the block.  x, the label bytes, the taps,
// the three band tables, the histogram clear and the summary epilogue happen once; per member the thread's 16 r_k values (requested before that
// member's plane walk and used after it, as the single map's are), the walk over m_k's latent planes through the same ms / T1 buffers, and s = s + e_k w_k in member order
// (s = a_0 for the first).  The map is a = s inv_K, one fp32 multiply; the summaries are taken over a.  K and every loop bound are uniform over the block.
#include "anomaly_summary.h"

namespace sa {

constexpr int AN_TW = 32, AN_TH = 8, AN_LD = 16;      // tile: W x H voxels (one column per thread), planes per run (16: 61 us against 79 for 8 on a
                                                      // 160 x 224 x 160 volume, same call; 32 would leave 700 blocks for 256 CUs)
static_assert(AN_TW * AN_TH == AN_THREADS, "one (h, w) column per thread of the summary's block (anomaly_summary.h)");
constexpr int AN_TAPS = 2 * SA_ANOMALY_MAX_R + 1;

struct AnGeom {
    int D, H, W, d, h, w, fD, fH, fW, R;
    int tiles_h, tiles_w, chunks, nblk;      // blocks per volume
    int nDm, nHm, nWm;                       // most latent cells a block's run / tile can see per axis (LDS strides)
    int mode, has_t;
    float inv_bin, t;
};
struct AnTaps { float g[AN_TAPS]; };

// most cells of size f that L consecutive voxels can touch, capped by the cells there are
static int an_span_cells(int L, int f, int cells) {
    const int n = (L + f - 2) / f + 1;
    return n < cells ? n : cells;
}
static int64_t an_align(int64_t v) { return (v + 15) & ~(int64_t)15; }
// dynamic LDS in bytes: taps, A_D [nDm][LD], A_H [nHm][TH], A_W [nWm][TW], the latent plane's neighbourhood [nHm][nWm], its W-filtered rows [nHm][TW],
// the 2 x 256 histogram, per wave one fp64, one fp32 and five counts
static int64_t an_lds_floats(const AnGeom& g) {
    return 64 + (int64_t)g.nDm * AN_LD + (int64_t)g.nHm * AN_TH + (int64_t)g.nWm * AN_TW + (int64_t)g.nHm * g.nWm + (int64_t)g.nHm * AN_TW;
}
static int64_t an_lds_bytes(const AnGeom& g) { return an_align(an_lds_floats(g) * 4) + AN_TAIL_BYTES; }

// A[p][c]: the taps of voxel p's window that fall into cell c, added in ascending order (at most min(f, 2R + 1) of them)
__device__ __forceinline__ float an_band(const float* gs, int R, int p, int c, int f) {
    const int lo = max(-R, c * f - p), hi = min(R, c * f + f - 1 - p);
    float s = 0.f;
    for (int t = lo; t <= hi; ++t) s += gs[t + R];
    return s;
}

// members of an ensemble: member k's r and m start k * r_stride and k * m_stride elements after the first one's; inv_K = (float)(1.0 / K) from the host
struct AnMembers {
    int K;
    float inv_K;
    int64_t r_stride, m_stride;
};

// ENS = false: one (r, m), the code of sa_anomaly_map (M is not read); ENS = true: the loop over M.K members
template <bool ENS>
__device__ __forceinline__ void anomaly_map_body(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ m,
                                                 const unsigned char* __restrict__ label, float* __restrict__ a_out, const AnGeom& g, const AnTaps& taps,
                                                 unsigned long long* __restrict__ part, unsigned long long* __restrict__ results, const AnMembers& M) {
    extern __shared__ __attribute__((aligned(16))) char an_smem[];
    float* gs = reinterpret_cast<float*>(an_smem);
    float* AD = gs + 64;
    float* AH = AD + g.nDm * AN_LD;
    float* AW = AH + g.nHm * AN_TH;
    float* ms = AW + g.nWm * AN_TW;
    float* T1 = ms + g.nHm * g.nWm;
    const int64_t nfl = 64 + (int64_t)g.nDm * AN_LD + (int64_t)g.nHm * AN_TH + (int64_t)g.nWm * AN_TW + (int64_t)g.nHm * g.nWm + (int64_t)g.nHm * AN_TW;
    char* tail = an_smem + ((nfl * 4 + 15) & ~(int64_t)15);
    const AnTail T = an_tail(tail);      // the summary's histogram and wave slots (anomaly_summary.h)
    uint32_t* hist = T.hist;

    const int tid = threadIdx.x, wl = tid % AN_TW, hl = tid / AN_TW;
    const int64_t b = blockIdx.y;
    int blk = blockIdx.x;
    const int tw = blk % g.tiles_w; blk /= g.tiles_w;
    const int th = blk % g.tiles_h;
    const int chunk = blk / g.tiles_h;
    const int w0 = tw * AN_TW, h0 = th * AN_TH, p0 = chunk * AN_LD;
    const int np = min(AN_LD, g.D - p0);
    const bool valid = h0 + hl < g.H && w0 + wl < g.W;
    const int64_t plane = (int64_t)g.H * g.W;
    const int64_t base = (b * g.D + p0) * plane + (int64_t)(h0 + hl) * g.W + (w0 + wl);

    hist[tid] = 0u;
    hist[tid + AN_THREADS] = 0u;

    // this thread's voxels: in flight while the weights are made
    float xv[AN_LD], rv[AN_LD];
    unsigned char lv[AN_LD];
#pragma unroll
    for (int k = 0; k < AN_LD; ++k) {
        const bool ok = valid && k < np;
        xv[k] = ok ? x[base + k * plane] : 0.f;
        rv[k] = ok ? r[base + k * plane] : 0.f;
        lv[k] = (ok && label) ? label[base + k * plane] : (unsigned char)0;
    }

    float wacc[AN_LD];
#pragma unroll
    for (int k = 0; k < AN_LD; ++k) wacc[k] = 0.f;
    // ensembles only: the running sum s, the loads of member km's r (in flight under its own walk, as the first member's are) and the step that closes it
    [[maybe_unused]] float sacc[AN_LD] = {};
    [[maybe_unused]] auto load_member = [&](int km) {      // (one pointer stepped from plane to plane: 16 addresses kept across the member loop cost 32 VGPRs)
        if (km == 0) return;                               // (the first member's came with x)
        const float* p = r + (km * M.r_stride + base);
#pragma unroll
        for (int k = 0; k < AN_LD; ++k, p += plane) rv[k] = (valid && k < np) ? *p : 0.f;
    };
    [[maybe_unused]] auto fold = [&](int km) {      // s = a_0, then s = s + a_k with a_k the number sa_anomaly_map computes for member k
#pragma unroll
        for (int k = 0; k < AN_LD; ++k) {
            const float dlt = xv[k] - rv[k];
            const float e = g.mode == SA_ANOMALY_ABS ? fabsf(dlt) : g.mode == SA_ANOMALY_POSITIVE ? fmaxf(dlt, 0.f) : fmaxf(-dlt, 0.f);
            const float a = m ? e * wacc[k] : e;
            sacc[k] = km == 0 ? a : sacc[k] + a;
            wacc[k] = 0.f;
        }
    };
    if (m) {
        const int R = g.R;
        for (int i = tid; i < 2 * R + 1; i += AN_THREADS) gs[i] = taps.g[i];
        // the latent cells this run / tile can see: those that hold a voxel of [first - R, last + R] inside the volume
        const int cD0 = max(p0 - R, 0) / g.fD, nD = min(g.D - 1, p0 + AN_LD - 1 + R) / g.fD - cD0 + 1;
        const int cH0 = max(h0 - R, 0) / g.fH, nH = min(g.H - 1, h0 + AN_TH - 1 + R) / g.fH - cH0 + 1;
        const int cW0 = max(w0 - R, 0) / g.fW, nW = min(g.W - 1, w0 + AN_TW - 1 + R) / g.fW - cW0 + 1;
        __syncthreads();
        for (int e = tid; e < nD * AN_LD; e += AN_THREADS) {
            const int j = e / AN_LD, k = e % AN_LD;
            AD[e] = p0 + k < g.D ? an_band(gs, R, p0 + k, cD0 + j, g.fD) : 0.f;
        }
        for (int e = tid; e < nH * AN_TH; e += AN_THREADS) {
            const int j = e / AN_TH, k = e % AN_TH;
            AH[e] = h0 + k < g.H ? an_band(gs, R, h0 + k, cH0 + j, g.fH) : 0.f;
        }
        for (int e = tid; e < nW * AN_TW; e += AN_THREADS) {
            const int j = e / AN_TW, k = e % AN_TW;
            AW[e] = w0 + k < g.W ? an_band(gs, R, w0 + k, cW0 + j, g.fW) : 0.f;
        }
        const int members = ENS ? M.K : 1;
        for (int km = 0; km < members; ++km) {
            if constexpr (ENS) load_member(km);
            // (a later member's first plane is the next plane of the two-barrier pattern below: ms and T1 are free again after the second barrier)
            const float* mb = m + (ENS ? km * M.m_stride : (int64_t)0) + b * ((int64_t)g.d * g.h * g.w);
            for (int j = 0; j < nD; ++j) {
                // (cD0 + j < d, cH0 + ih < h, cW0 + iw < w by the construction of nD, nH, nW)
                for (int e = tid; e < nH * nW; e += AN_THREADS) {
                    const int ih = e / nW, iw = e - ih * nW;
                    ms[ih * g.nWm + iw] = mb[((int64_t)(cD0 + j) * g.h + (cH0 + ih)) * g.w + (cW0 + iw)];
                }
                __syncthreads();      // (the first pass: the band tables too)
                for (int e = tid; e < nH * AN_TW; e += AN_THREADS) {
                    const int ih = e / AN_TW, c = e % AN_TW;
                    float acc = 0.f;
                    for (int iw = 0; iw < nW; ++iw) acc = fmaf(AW[iw * AN_TW + c], ms[ih * g.nWm + iw], acc);
                    T1[e] = acc;
                }
                __syncthreads();
                float s = 0.f;
                for (int ih = 0; ih < nH; ++ih) s = fmaf(AH[ih * AN_TH + hl], T1[ih * AN_TW + wl], s);
#pragma unroll
                for (int k = 0; k < AN_LD; ++k) wacc[k] = fmaf(AD[j * AN_LD + k], s, wacc[k]);
            }
            if constexpr (ENS) fold(km);
        }
    } else {
        __syncthreads();          // the histogram is clear
        if constexpr (ENS) {
            for (int km = 0; km < M.K; ++km) {
                load_member(km);
                fold(km);
            }
        }
    }

    AnAcc acc;
#pragma unroll
    for (int k = 0; k < AN_LD; ++k) {
        if (valid && k < np) {
            const float dlt = xv[k] - rv[k];
            const float e = g.mode == SA_ANOMALY_ABS ? fabsf(dlt) : g.mode == SA_ANOMALY_POSITIVE ? fmaxf(dlt, 0.f) : fmaxf(-dlt, 0.f);
            const float a = ENS ? sacc[k] * M.inv_K : m ? e * wacc[k] : e;
            a_out[base + k * plane] = a;
            an_account(acc, hist, a, lv[k] != 0 ? 1u : 0u, g.inv_bin, g.has_t != 0, g.t);
        }
    }
    an_block_finish(acc, T, part + (b * g.nblk + blockIdx.x) * AN_PART, results + b * AN_WORDS);
}

__global__ __launch_bounds__(AN_THREADS) void anomaly_map_kernel(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ m,
                                                                 const unsigned char* __restrict__ label, float* __restrict__ a_out, const AnGeom g,
                                                                 const AnTaps taps, unsigned long long* __restrict__ part,
                                                                 unsigned long long* __restrict__ results) {
    anomaly_map_body<false>(x, r, m, label, a_out, g, taps, part, results, AnMembers{1, 1.f, 0, 0});
}

__global__ __launch_bounds__(AN_THREADS) void anomaly_map_ensemble_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                                          const float* __restrict__ m, const unsigned char* __restrict__ label,
                                                                          float* __restrict__ a_out, const AnGeom g, const AnTaps taps,
                                                                          unsigned long long* __restrict__ part,
                                                                          unsigned long long* __restrict__ results, const AnMembers M) {
    anomaly_map_body<true>(x, r, m, label, a_out, g, taps, part, results, M);
}

// one block per volume adds the blocks' partial words in a fixed order (an_finish_body, anomaly_summary.h)
__global__ __launch_bounds__(256) void anomaly_finish_kernel(const unsigned long long* __restrict__ part, int nblk, unsigned long long* __restrict__ results) {
    an_finish_body(part, nblk, results);
}

}  // namespace sa

using namespace sa;

namespace {

// SA_EINVAL for what the rule refuses (a side that its latent side does not divide, R outside 0..24, a residual mode it does not know, inv_bin <= 0);
// SA_EUNSUPPORTED for what this kernel does not cover (B > 65535, a volume of 2^31 voxels or more, a tile neighbourhood beyond 64 KiB of LDS)
int an_plan(const sa_anomaly_params& P, bool weighted, AnGeom& g) {
    if (P.B < 1 || P.D < 1 || P.H < 1 || P.W < 1) return SA_EINVAL;
    if (P.residual != SA_ANOMALY_ABS && P.residual != SA_ANOMALY_POSITIVE && P.residual != SA_ANOMALY_NEGATIVE) return SA_EINVAL;
    if (P.R < 0 || P.R > SA_ANOMALY_MAX_R) return SA_EINVAL;
    if (!(P.inv_bin > 0.f) || P.inv_bin - P.inv_bin != 0.f) return SA_EINVAL;
    if (P.has_threshold && P.threshold - P.threshold != 0.f) return SA_EINVAL;
    g.D = P.D; g.H = P.H; g.W = P.W;
    g.d = g.h = g.w = g.fD = g.fH = g.fW = 1;
    if (weighted) {
        if (P.d < 1 || P.h < 1 || P.w < 1 || P.D % P.d || P.H % P.h || P.W % P.w) return SA_EINVAL;
        g.d = P.d; g.h = P.h; g.w = P.w;
        g.fD = P.D / P.d; g.fH = P.H / P.h; g.fW = P.W / P.w;
    }
    g.R = P.R;
    if (P.B > 65535) return SA_EUNSUPPORTED;
    const int64_t vol = (int64_t)P.D * P.H * P.W;
    if (vol >= 0x7fffffffll) return SA_EUNSUPPORTED;
    g.tiles_h = (P.H + AN_TH - 1) / AN_TH;
    g.tiles_w = (P.W + AN_TW - 1) / AN_TW;
    g.chunks = (P.D + AN_LD - 1) / AN_LD;
    const int64_t nblk = (int64_t)g.tiles_h * g.tiles_w * g.chunks;      // <= vol
    g.nblk = (int)nblk;
    g.nDm = weighted ? an_span_cells(AN_LD + 2 * P.R, g.fD, g.d) : 0;
    g.nHm = weighted ? an_span_cells(AN_TH + 2 * P.R, g.fH, g.h) : 0;
    g.nWm = weighted ? an_span_cells(AN_TW + 2 * P.R, g.fW, g.w) : 0;
    if (an_lds_bytes(g) > 65536) return SA_EUNSUPPORTED;      // (R <= 24 keeps it below 44 KiB: 56 x 80 cells at f = 1)
    g.mode = P.residual;
    g.has_t = P.has_threshold != 0;
    g.inv_bin = P.inv_bin;
    g.t = P.threshold;
    return 0;
}

}  // namespace

extern "C" int64_t sa_anomaly_map_workspace_bytes(const sa_anomaly_params* params) {
    if (!params) return SA_EINVAL;
    AnGeom g;
    const int rc = an_plan(*params, params->d > 0, g);
    return rc ? rc : (int64_t)params->B * g.nblk * AN_PART * 8;
}

extern "C" int sa_anomaly_map(const float* x, const float* r, const float* m, const unsigned char* label, float* a_out,
                              const sa_anomaly_params* params, void* results, void* ws, void* stream) {
    if (!x || !r || !a_out || !params || !results || !ws || (((uintptr_t)results) & 7u) != 0 || (((uintptr_t)ws) & 7u) != 0) return SA_EINVAL;
    AnGeom g;
    const int rc = an_plan(*params, m != nullptr, g);
    if (rc) return rc;
    AnTaps taps;
    for (int i = 0; i < AN_TAPS; ++i) taps.g[i] = i < 2 * params->R + 1 ? params->taps[i] : 0.f;
    hipStream_t st = (hipStream_t)stream;
    const int B = params->B;
    if (hipMemsetAsync(results, 0, (size_t)B * AN_WORDS * 8, st) != hipSuccess) {
        g_last_error = hipGetLastError();
        return (int)g_last_error;
    }
    SA_LAUNCH(anomaly_map_kernel, dim3((unsigned)g.nblk, (unsigned)B), dim3(AN_THREADS), (size_t)an_lds_bytes(g), st, x, r, m, label, a_out, g, taps,
              (unsigned long long*)ws, (unsigned long long*)results);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(anomaly_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, (const unsigned long long*)ws, g.nblk, (unsigned long long*)results);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_anomaly_map_ensemble(const float* x, const float* r, int64_t r_member_stride, const float* m, int64_t m_member_stride,
                                       const unsigned char* label, float* a_out, const sa_anomaly_params* params, int members, void* results, void* ws,
                                       void* stream) {
    if (!x || !r || !a_out || !params || !results || !ws || (((uintptr_t)results) & 7u) != 0 || (((uintptr_t)ws) & 7u) != 0) return SA_EINVAL;
    if (members < 1 || members > SA_ANOMALY_MAX_MEMBERS) return SA_EINVAL;
    AnGeom g;
    const int rc = an_plan(*params, m != nullptr, g);
    if (rc) return rc;
    const int B = params->B;
    // a member's extent in elements (an_plan: B <= 65535, D H W < 2^31, d h w <= D H W)
    if (r_member_stride < (int64_t)B * g.D * g.H * g.W) return SA_EINVAL;
    if (m && m_member_stride < (int64_t)B * g.d * g.h * g.w) return SA_EINVAL;
    AnTaps taps;
    for (int i = 0; i < AN_TAPS; ++i) taps.g[i] = i < 2 * params->R + 1 ? params->taps[i] : 0.f;
    const AnMembers M{members, (float)(1.0 / (double)members), r_member_stride, m ? m_member_stride : (int64_t)0};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(results, 0, (size_t)B * AN_WORDS * 8, st) != hipSuccess) {
        g_last_error = hipGetLastError();
        return (int)g_last_error;
    }
    SA_LAUNCH(anomaly_map_ensemble_kernel, dim3((unsigned)g.nblk, (unsigned)B), dim3(AN_THREADS), (size_t)an_lds_bytes(g), st, x, r, m, label, a_out, g,
              taps, (unsigned long long*)ws, (unsigned long long*)results, M);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(anomaly_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, (const unsigned long long*)ws, g.nblk, (unsigned long long*)results);
    SA_CHECK_LAUNCH();
    return 0;
}
