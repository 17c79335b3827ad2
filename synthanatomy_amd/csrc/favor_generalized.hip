// Generalized (ReLU) attention of the Performer: the random-feature map FastAttention uses with generalized_attention=True, kernel_fn = nn.ReLU().
// A restatement of performer-pytorch 1.0.11 generalized_kernel (the package is not pinned by the reference and was not at hand: unpinned, like the rest
// of the layer stack).  With c = dim_head^-1/4 and P [m][dim_head] the projection matrix (the callers fold c into P):
//
//     dd = (c x) P^T        phi(x) = relu(dd) + 1e-3        the same map for queries and keys
//
// There is no m^-1/2 ratio, no -|x|^2 c^2 / 2 term and no row or global maximum, so nothing is reduced across rows and q and k can share a launch.
// Feature columns [m, LDF) are written as ZERO (not 1e-3): the causal scans sum over LDF columns.
// Derivative: d dd = d phi * [phi > 1e-3f], a strict fp32 comparison on the STORED feature -- the backward kernels read the mask from phi and never see
// dd, so the tape keeps one tensor per side.  relu(dd) + 1e-3f rounds to exactly 1e-3f for 0 < dd < ~6e-11 (half an ulp of 1e-3f), so this mask differs
// from [dd > 0] only there.
//
//   fp32 parity mode : gen_feat_fwd / gen_feat_bwd, elementwise around the exact-fp32 projection GEMMs of the engine
//   throughput mode  : gen_project_fwd / gen_project_bwd, the HBM-bound split-bf16 projection kernels of favor_proj.hip with the map (its mask) applied
//                      to the accumulators (the operand rows): dd and d loss / d dd never exist
//   decoding         : gen_step_proj + gen_step, the O(N) state update of one position (no stabiliser state: E and Ez are plain running sums)
//
// No atomics anywhere: every output element is written by one thread in a fixed order, results are bitwise repeatable.
#include "favor_proj_common.h"

namespace sa {

constexpr float GEN_EPS = 1e-3f;   // generalized_kernel's kernel_epsilon

__device__ __forceinline__ float gen_phi(float dd) { return (dd < 0.f ? 0.f : dd) + GEN_EPS; }
// d dd of one element: the mask is read from the stored feature; `in` = the column is a feature column (< m) of a valid row
__device__ __forceinline__ float gen_dphi(bool in, float phi, float dphi) { return (in & (phi > GEN_EPS)) ? dphi : 0.f; }

// ---- fp32 parity mode: one thread per 16-byte piece of a [rows][LDF] matrix
__global__ __launch_bounds__(256) void gen_feat_fwd_kernel(const float* __restrict__ dd, float* __restrict__ feat, int64_t n4, int m, int LDF) {
    const int per_row = LDF >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % per_row) * 4;
        const float4 v = *(const float4*)(dd + i * 4);
        *(float4*)(feat + i * 4) = make_float4(c < m ? gen_phi(v.x) : 0.f, c + 1 < m ? gen_phi(v.y) : 0.f, c + 2 < m ? gen_phi(v.z) : 0.f,
                                               c + 3 < m ? gen_phi(v.w) : 0.f);
    }
}

__global__ __launch_bounds__(256) void gen_feat_bwd_kernel(const float* __restrict__ dfeat, const float* __restrict__ feat, float* __restrict__ ddd, int64_t n4,
                                                           int m, int LDF) {
    const int per_row = LDF >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % per_row) * 4;
        const float4 g = *(const float4*)(dfeat + i * 4), f = *(const float4*)(feat + i * 4);
        *(float4*)(ddd + i * 4) = make_float4(gen_dphi(c < m, f.x, g.x), gen_dphi(c + 1 < m, f.y, g.y), gen_dphi(c + 2 < m, f.z, g.z), gen_dphi(c + 3 < m, f.w, g.w));
    }
}

// ---- throughput mode.  blockIdx.y = operand (0: q, 1: k): operand gi is read x_goff and written f_goff ELEMENTS behind operand 0
struct GenProjArgs {
    const float* x;        // forward: rows of 64 floats, head blocks of wider rows (proj_row_off)
    const float* proj;     // [m][64], data normaliser folded in
    float* feat;           // forward: phi [rows][LDF]
    const float *dfeat, *pfeat;   // adjoint: d phi and the stored phi [rows][LDF]
    float* dx;             // adjoint: head blocks of wider rows
    int64_t rows, x_goff, f_goff;
    int32_t m, LDF, x_stride, heads;
};

// forward: favor_project_fwd_kernel's block (128 rows, wave = 32 rows, D[i = feature][j = row]); phi leaves the accumulators as 16-byte pieces
__global__ __launch_bounds__(256, 2) void gen_project_fwd_kernel(const GenProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nfr = a.LDF >> 4;
    unsigned char* const sPh = smem;
    unsigned char* const sPl = smem + nfr * 16 * 128;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), qi = lane & 15, g = lane >> 4;
    const float* const x = a.x + (int64_t)blockIdx.y * a.x_goff;
    float* const feat = a.feat + (int64_t)blockIdx.y * a.f_goff;
    const int64_t r0 = (int64_t)blockIdx.x * 128 + w * 32;
    short8_t xh[2][2], xl[2][2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        const int64_t r = r0 + st * 16 + qi;
        const bool ok = r < a.rows;
        const float* xr = x + proj_row_off(ok ? r : a.rows - 1, a.heads, a.x_stride);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float4 v0 = proj_keep(*(const float4*)(xr + ks * 32 + g * 8), ok), v1 = proj_keep(*(const float4*)(xr + ks * 32 + g * 8 + 4), ok);
            const float xs[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            split8(xs, xh[st][ks], xl[st][ks]);
        }
    }
    proj_stage(sPh, sPl, a.proj, a.m, nfr * 16, tid);
    __syncthreads();
    float* o0 = feat + (r0 + qi) * a.LDF + g * 4;
    float* o1 = o0 + (int64_t)16 * a.LDF;
    const bool ok0 = r0 + qi < a.rows, ok1 = r0 + 16 + qi < a.rows;
    for (int f = 0; f < nfr; ++f) {
        short8_t ah[2], al[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const uint32_t o = lroff(f * 16 + qi, ks * 32 + g * 8);
            ah[ks] = *(const short8_t*)(sPh + o);
            al[ks] = *(const short8_t*)(sPl + o);
        }
        float4_t c0 = (float4_t){0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            c0 = mfma3(ah[ks], al[ks], xh[0][ks], xl[0][ks], c0);
            c1 = mfma3(ah[ks], al[ks], xh[1][ks], xl[1][ks], c1);
        }
        float e0[4], e1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool in = f * 16 + g * 4 + r < a.m;
            e0[r] = in ? gen_phi(c0[r]) : 0.f;
            e1[r] = in ? gen_phi(c1[r]) : 0.f;
        }
        if (ok0) *(float4*)(o0 + f * 16) = make_float4(e0[0], e0[1], e0[2], e0[3]);
        if (ok1) *(float4*)(o1 + f * 16) = make_float4(e1[0], e1[1], e1[2], e1[3]);
    }
}

// adjoint: dx[r][d] = sum_{f < m} d phi[r][f] [phi[r][f] > 1e-3f] P[f][d]; favor_project_bwd_kernel's block (128 rows, wave = 2 x 16 rows, D[i = d][j = row],
// transposing reads of the permuted tile).  The mask is applied to the operand rows as they arrive, 32-feature block by block (three blocks of both tensors in
// flight per lane); columns >= m are dropped by the column test, whatever d phi holds there.
__global__ __launch_bounds__(256, 2) void gen_project_bwd_kernel(const GenProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nks = (a.LDF + 31) >> 5;
    unsigned char* const sPh = smem;
    unsigned char* const sPl = smem + nks * 32 * 128;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), qi = lane & 15, g = lane >> 4;
    const float* const dfeat = a.dfeat + (int64_t)blockIdx.y * a.f_goff;
    const float* const pfeat = a.pfeat + (int64_t)blockIdx.y * a.f_goff;
    float* const dx = a.dx + (int64_t)blockIdx.y * a.x_goff;
    proj_stage<true>(sPh, sPl, a.proj, a.m, nks * 32, tid);
    __syncthreads();
    const uint32_t trow = (uint32_t)g * 4u + ((uint32_t)qi >> 2), tcol = (uint32_t)(qi & 3) * 4u;
    for (int it = 0; it < 2; ++it) {
        const int64_t r = (int64_t)blockIdx.x * 128 + w * 32 + it * 16 + qi;
        const bool ok = r < a.rows;
        const int64_t rc = ok ? r : a.rows - 1;
        const float* pg = dfeat + rc * a.LDF;
        const float* pf = pfeat + rc * a.LDF;
        float4_t acc[4];
#pragma unroll
        for (int df = 0; df < 4; ++df) acc[df] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int grp = 0; grp < 3; ++grp) {
            float4 vg[3][2], vf[3][2];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int c = min((grp * 3 + k) * 32 + g * 8 + q * 4, a.LDF - 4);   // eight consecutive features per lane (permuted tile rows)
                    vg[k][q] = *(const float4*)(pg + c);
                    vf[k][q] = *(const float4*)(pf + c);
                }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int ks = grp * 3 + k;
                if (ks < nks) {
                    float xs[8];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int c0 = ks * 32 + g * 8 + q * 4;
                        const float g4[4] = {vg[k][q].x, vg[k][q].y, vg[k][q].z, vg[k][q].w}, f4[4] = {vf[k][q].x, vf[k][q].y, vf[k][q].z, vf[k][q].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) xs[q * 4 + e] = gen_dphi(ok & (c0 + e < a.m), f4[e], g4[e]);
                    }
                    short8_t bh, bl;
                    split8(xs, bh, bl);
#pragma unroll
                    for (int df = 0; df < 4; ++df) {
                        const uint32_t o0 = lroff(ks * 32 + trow, df * 16 + tcol), o1 = lroff(ks * 32 + 16 + trow, df * 16 + tcol);
                        const short8_t ah = __builtin_shufflevector(lds_tr16_b64(sPh + o0), lds_tr16_b64(sPh + o1), 0, 1, 2, 3, 4, 5, 6, 7);
                        const short8_t al = __builtin_shufflevector(lds_tr16_b64(sPl + o0), lds_tr16_b64(sPl + o1), 0, 1, 2, 3, 4, 5, 6, 7);
                        acc[df] = mfma3(ah, al, bh, bl, acc[df]);
                    }
                }
            }
        }
        if (ok) {
            float* dxr = dx + proj_row_off(r, a.heads, a.x_stride);
#pragma unroll
            for (int df = 0; df < 4; ++df) *(float4*)(dxr + df * 16 + g * 4) = make_float4(acc[df][0], acc[df][1], acc[df][2], acc[df][3]);
        }
    }
}

// ---- decoding: one position of the global heads, one block per (batch, head)
struct GenStepArgs {
    const float *q, *k, *v;            // rows of the fused qkv output
    const float* proj;                 // [m][64], data normaliser folded in
    int q_stride, q_off, k_stride, k_off, v_stride, v_off;
    int G, dh, m, LDF;
    int64_t rows;                      // B * G
    float* dd;                         // [2][B*G][LDF] scratch: phi(q_t) | phi(k_t)
    float *E, *Ez;                     // state [B*G][LDF][dh], [B*G][LDF]: plain running sums, zero at the start
    float* out;                        // attention output rows
    int out_stride, out_off;
    float eps_den;
};

// phi(q_t) and phi(k_t) of the block's head: favor_step_proj_body's dot products (the 16 pieces of a projection row are fetched before the fma chain)
__global__ __launch_bounds__(256) void gen_step_proj_kernel(const GenStepArgs a) {
    __shared__ float sq[64], sk[64];
    const int bg = (int)blockIdx.x, b = bg / a.G, g = bg % a.G, tid = threadIdx.x;
    if (tid < 64) {
        sq[tid] = a.q[(int64_t)b * a.q_stride + a.q_off + g * 64 + tid];
        sk[tid] = a.k[(int64_t)b * a.k_stride + a.k_off + g * 64 + tid];
    }
    __syncthreads();
    for (int e = tid; e < a.LDF; e += 256) {
        float fq = 0.f, fk = 0.f;
        if (e < a.m) {
            const float4* pr = (const float4*)(a.proj + (int64_t)e * 64);
            float4 pv[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) pv[i] = pr[i];
            float aq = 0.f, ak = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int d = 4 * i;
                aq = fmaf(sq[d], pv[i].x, fmaf(sq[d + 1], pv[i].y, fmaf(sq[d + 2], pv[i].z, fmaf(sq[d + 3], pv[i].w, aq))));
                ak = fmaf(sk[d], pv[i].x, fmaf(sk[d + 1], pv[i].y, fmaf(sk[d + 2], pv[i].z, fmaf(sk[d + 3], pv[i].w, ak))));
            }
            fq = gen_phi(aq);
            fk = gen_phi(ak);
        }
        a.dd[(int64_t)bg * a.LDF + e] = fq;
        a.dd[(a.rows + bg) * a.LDF + e] = fk;
    }
}

// E += phi(k_t) (x) v_t, Ez += phi(k_t), out = (phi(q_t) . E) / (phi(q_t) . (Ez + eps)) -- the denominator of sa_favor_scan_a_norm (den_eps added to the
// running key sums before the dot product).  16 waves: wave w owns features w, w + 16, ... (17 of them for LDF <= 272), lane = value dimension, as in
// favor_step_body: all of a wave's state rows are in flight together.
__global__ __launch_bounds__(1024) void gen_step_kernel(const GenStepArgs a) {
    __shared__ float sv[64], sqf[272], skf[272], red[16], snum[16][64];
    const int bg = (int)blockIdx.x, b = bg / a.G, g = bg % a.G, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = a.m;
    float* const E = a.E + (int64_t)bg * a.LDF * 64;
    float ev[17];
#pragma unroll
    for (int it = 0; it < 17; ++it) {
        const int e = wv + 16 * it;
        ev[it] = e < m ? E[e * 64 + lane] : 0.f;
    }
    const float qf = tid < m ? a.dd[(int64_t)bg * a.LDF + tid] : 0.f;
    const float kf = tid < m ? a.dd[(a.rows + bg) * a.LDF + tid] : 0.f;
    const float ez = tid < m ? a.Ez[(int64_t)bg * a.LDF + tid] : 0.f;
    if (tid < 64) sv[tid] = a.v[(int64_t)b * a.v_stride + a.v_off + g * 64 + tid];
    float den = 0.f;
    if (tid < m) {
        sqf[tid] = qf;
        skf[tid] = kf;
        const float z = ez + kf;
        a.Ez[(int64_t)bg * a.LDF + tid] = z;
        den = qf * (z + a.eps_den);
    }
    den = wave_sum(den);
    if (lane == 0) red[wv] = den;
    __syncthreads();
    float num = 0.f;
#pragma unroll
    for (int it = 0; it < 17; ++it) {
        const int e = wv + 16 * it;
        if (e < m) {
            const float x = fmaf(skf[e], sv[lane], ev[it]);
            E[e * 64 + lane] = x;
            num = fmaf(sqf[e], x, num);
        }
    }
    snum[wv][lane] = num;
    __syncthreads();
    if (tid < 64) {
        den = 0.f;
        num = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            den += red[w];
            num += snum[w][tid];
        }
        a.out[(int64_t)b * a.out_stride + a.out_off + g * 64 + tid] = num / den;
    }
}

static int gen_elementwise_grid(int64_t n4) { return (int)std::min<int64_t>((n4 + 255) / 256, 256 * 16); }

}  // namespace sa

using namespace sa;

extern "C" int sa_favor_generalized_features_fwd(const float* dd, float* feat, int64_t rows, int m, int LDF, void* stream) {
    if (!dd || !feat || rows <= 0 || m <= 0 || LDF <= 0) return SA_EINVAL;
    if ((LDF & 3) || LDF < m) return SA_EUNSUPPORTED;
    const int64_t n4 = rows * (LDF >> 2);
    SA_LAUNCH(gen_feat_fwd_kernel, dim3(gen_elementwise_grid(n4)), dim3(256), 0, (hipStream_t)stream, dd, feat, n4, m, LDF);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_favor_generalized_features_bwd(const float* dfeat, const float* feat, float* ddd, int64_t rows, int m, int LDF, void* stream) {
    if (!dfeat || !feat || !ddd || rows <= 0 || m <= 0 || LDF <= 0) return SA_EINVAL;
    if ((LDF & 3) || LDF < m) return SA_EUNSUPPORTED;
    const int64_t n4 = rows * (LDF >> 2);
    SA_LAUNCH(gen_feat_bwd_kernel, dim3(gen_elementwise_grid(n4)), dim3(256), 0, (hipStream_t)stream, dfeat, feat, ddd, n4, m, LDF);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_favor_generalized_project_features(const float* x, int x_stride, int heads, const float* proj, float* feat, int64_t rows, int m, int LDF,
                                                     int dh, int ngroups, int64_t x_goff, int64_t feat_goff, void* stream) {
    if (!x || !proj || !feat || rows <= 0 || m <= 0 || heads <= 0 || ngroups <= 0) return SA_EINVAL;
    if (dh != 64 || (LDF & 15) || LDF < m || LDF > 272 || (x_stride & 3) || x_stride < dh * heads || ngroups > 2 || (x_goff & 3) || (feat_goff & 3))
        return SA_EUNSUPPORTED;
    GenProjArgs a = {};
    a.x = x; a.proj = proj; a.feat = feat; a.rows = rows; a.m = m; a.LDF = LDF; a.x_stride = x_stride; a.heads = heads; a.x_goff = x_goff; a.f_goff = feat_goff;
    const size_t lds = (size_t)2 * LDF * 128;
    hipFuncSetAttribute((const void*)gen_project_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    SA_LAUNCH(gen_project_fwd_kernel, dim3((unsigned)((rows + 127) / 128), ngroups), dim3(256), lds, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_favor_generalized_project_bwd(const float* dfeat, const float* feat, const float* proj, float* dx, int dx_stride, int heads, int64_t rows,
                                                int m, int LDF, int dh, int ngroups, int64_t feat_goff, int64_t dx_goff, void* stream) {
    if (!dfeat || !feat || !proj || !dx || rows <= 0 || m <= 0 || heads <= 0 || ngroups <= 0) return SA_EINVAL;
    if (dh != 64 || (LDF & 15) || LDF < m || LDF > 272 || (dx_stride & 3) || dx_stride < dh * heads || ngroups > 2 || (dx_goff & 3) || (feat_goff & 3))
        return SA_EUNSUPPORTED;
    GenProjArgs a = {};
    a.dfeat = dfeat; a.pfeat = feat; a.proj = proj; a.dx = dx; a.rows = rows; a.m = m; a.LDF = LDF; a.x_stride = dx_stride; a.heads = heads;
    a.x_goff = dx_goff; a.f_goff = feat_goff;
    const size_t lds = (size_t)2 * ((LDF + 31) / 32) * 32 * 128;
    hipFuncSetAttribute((const void*)gen_project_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    SA_LAUNCH(gen_project_bwd_kernel, dim3((unsigned)((rows + 127) / 128), ngroups), dim3(256), lds, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}

extern "C" int sa_favor_generalized_step(const float* q, int q_stride, int q_off, const float* k, int k_stride, int k_off, const float* v, int v_stride,
                                         int v_off, const float* proj, int B, int G, int dh, int m, int LDF, float* dd, float* E, float* Ez, const int* pos,
                                         float* out, int out_stride, int out_off, void* stream) {
    if (!q || !k || !v || !proj || !dd || !E || !Ez || !pos || !out || B <= 0 || G <= 0 || dh <= 0 || m <= 0 || LDF <= 0) return SA_EINVAL;
    if (dh != 64 || m > 272 || LDF < m || LDF > 272) return SA_EUNSUPPORTED;   // 16 waves x 17 features
    GenStepArgs a = {};
    a.q = q; a.k = k; a.v = v; a.proj = proj;
    a.q_stride = q_stride; a.q_off = q_off; a.k_stride = k_stride; a.k_off = k_off; a.v_stride = v_stride; a.v_off = v_off;
    a.G = G; a.dh = dh; a.m = m; a.LDF = LDF; a.rows = (int64_t)B * G; a.dd = dd; a.E = E; a.Ez = Ez; a.out = out; a.out_stride = out_stride; a.out_off = out_off;
    a.eps_den = 1e-6f;
    SA_LAUNCH(gen_step_proj_kernel, dim3(B * G), dim3(256), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(gen_step_kernel, dim3(B * G), dim3(1024), 0, (hipStream_t)stream, a);
    SA_CHECK_LAUNCH();
    return 0;
}
