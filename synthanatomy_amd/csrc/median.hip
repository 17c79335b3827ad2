// Masked 3-D median filter of an anomaly map: sa_anomaly_median (include/synthanatomy_hip.h).  Per volume, with a the map, b an optional
// byte mask, e erosion steps and k in {1, 3, 5} the window's side:
//   m0 = [b != 0] (1 without a mask);   m(v) = AND of m0(v + t), |t|_1 <= e, false outside the volume;   a'(v) = m(v) ? a(v) : +0.0f
//   f(v) = the element of rank (k^3 - 1) / 2 among a'(v + t), t in [-k/2, k/2]^3, +0.0f outside the volume, in the order of the unsigned keys
//          key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000);   out(v) = m(v) ? f(v) : +0.0f
// and the summaries of sa_anomaly_map over out (anomaly_summary.h: the same device code fills the same record).
//
// Launches: a clear of the records; e erosion steps (median_erode_kernel: one byte per voxel, ping-pong between two workspace buffers, the first step
// reads the caller's mask; a step is m'(v) = m(v) and its six neighbours, a neighbour outside the volume being false -- e steps give the L1 ball);
// median_kernel<k>; the per-volume sums (median_finish_kernel).  Grid axis y is the volume: no block straddles volumes, and every address is formed
// from the voxel's own (d, h, w) inside its volume, so a window position outside the volume is the key of +0.0f and never the neighbouring volume's voxel.
//
// median_kernel<k>: a block owns an 8 x 16 x 32 (D x H x W) output tile.  It stages the keys of a' for the tile and a halo of k/2 voxels in LDS
// (12 x 20 x 36 words for k = 5), the select against the eroded mask done while staging, and takes the minimum and maximum key of everything it staged.
// All selection is on the integer keys (unsigned min / max / compare), which is the rule's total order exactly; floats are only read and written as bits.
//   - min == max over the block (a map is zero almost everywhere: outside the mask, far from resampled tokens): every window of the tile is constant,
//     f is that key, no window is read.
//   - otherwise every thread takes 16 voxels, a wave one 4 x 4 x 4 cube of the tile at a time; per voxel the k^3 keys go from LDS into registers (compile-time indices), with
//     their minimum and maximum; min == max ends it, and so do more than `rank` keys equal to the minimum (the rim of a blob); else the rank element is
//     found by bisection over the key bits BELOW the common prefix of min and max: ans = prefix; for bit = highest differing bit .. 0:
//     t = ans | 1 << bit; if #(key < t) <= rank then ans = t.  After all bits ans is the largest t with at most `rank` keys below it, the element of
//     that rank; the loop stops as soon as the interval it has narrowed down to holds ONE key (the counts on both sides are known), and the answer
//     is the smallest key >= ans.  One step costs k^3 compares and adds.
// Correctness does not depend on the early-outs: each returns what the bisection would.
#include "anomaly_summary.h"

namespace sa {

constexpr int MD_TD = SA_MEDIAN_TILE_D, MD_TH = SA_MEDIAN_TILE_H, MD_TW = SA_MEDIAN_TILE_W;
constexpr int MD_PER_THREAD = MD_TD * MD_TH * MD_TW / AN_THREADS;      // 16 voxels: the tile is 2 x 4 x 8 cubes of 4 x 4 x 4, a wave takes a cube per step
static_assert(MD_TD == 8 && MD_TH == 16 && MD_TW == 32 && MD_PER_THREAD == 16, "the thread -> voxel map below");
constexpr uint32_t MD_ZERO_KEY = 0x80000000u;      // the key of +0.0f

struct MdGeom {
    int D, H, W;
    int tiles_h, tiles_w, nblk;      // blocks per volume
    int has_t;
    float inv_bin, t;
};

__device__ __forceinline__ uint32_t md_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t md_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// one erosion step of a byte mask (any non-zero byte is foreground; the result is 0 / 1): grid (ceil(vol / 256), B)
__global__ __launch_bounds__(256) void median_erode_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int D, int H, int W) {
    const int64_t vol = (int64_t)D * H * W;                  // < 2^31 - 1 (md_plan), so the index and its divisions are 32-bit
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;      // (< vol + 256)
    if (i >= (uint32_t)vol) return;
    const uint32_t row = i / (uint32_t)W;
    const int w = (int)(i - row * (uint32_t)W), d = (int)(row / (uint32_t)H), h = (int)(row - (uint32_t)d * (uint32_t)H);
    const unsigned char* p = src + (int64_t)blockIdx.y * vol + i;
    const int64_t sh = W, sd = (int64_t)W * H;
    // (a neighbour is read only where it lies inside this volume)
    const bool ok = p[0] != 0 && w > 0 && p[-1] != 0 && w < W - 1 && p[1] != 0 && h > 0 && p[-sh] != 0 && h < H - 1 && p[sh] != 0 && d > 0 &&
                    p[-sd] != 0 && d < D - 1 && p[sd] != 0;
    dst[(int64_t)blockIdx.y * vol + i] = ok ? (unsigned char)1 : (unsigned char)0;
}

// the key of rank (K^3 - 1) / 2 of the K^3 window whose lowest corner is c (LDS, row stride LW, plane stride LH * LW)
template <int K, int LH, int LW>
__device__ __forceinline__ uint32_t md_select(const uint32_t* c) {
    constexpr int NK = K * K * K, RANK = (NK - 1) / 2;
    uint32_t w[NK];
#pragma unroll
    for (int z = 0; z < K; ++z)
#pragma unroll
        for (int y = 0; y < K; ++y)
#pragma unroll
            for (int x = 0; x < K; ++x) w[(z * K + y) * K + x] = c[(z * LH + y) * LW + x];
    uint32_t mn = w[0], mx = w[0];
#pragma unroll
    for (int i = 1; i < NK; ++i) {
        mn = min(mn, w[i]);
        mx = max(mx, w[i]);
    }
    if (mn == mx) return mn;
    // more than `rank` keys equal to the minimum: the rank element is the minimum (the rim of a blob in a map that is zero elsewhere; one pass instead
    // of up to 32, and a wave is as slow as its slowest lane)
    uint32_t lowest = 0u;
#pragma unroll
    for (int i = 0; i < NK; ++i) lowest += w[i] == mn ? 1u : 0u;
    if (lowest > (uint32_t)RANK) return mn;
    const int hb = 31 - __clz((int)(mn ^ mx));             // the highest bit in which two keys differ: every key has mn's bits above it
    uint32_t ans = mn & ~((2u << hb) - 1u);                // (hb = 31: 2u << 31 is 0, the prefix is empty)
    // invariant: lo = #(key < ans) <= rank < hi = #(key < ans + 2 << bit), so the rank element lies in [ans, ans + 2 << bit).  hi - lo == 1: it is the
    // only key there, no further bit is needed (continuous data: after about log2(k^3) + 2 steps instead of 27 to 32)
    uint32_t lo = 0u, hi = (uint32_t)NK;
    for (int bit = hb; bit >= 0 && hi - lo > 1u; --bit) {
        const uint32_t t = ans | (1u << bit);
        uint32_t below = 0u;
#pragma unroll
        for (int i = 0; i < NK; ++i) below += w[i] < t ? 1u : 0u;
        if (below <= (uint32_t)RANK) {
            ans = t;
            lo = below;
        } else {
            hi = below;
        }
    }
    // the smallest key >= ans: the rank element either way (after all bits every key in [ans, ans + 1) is ans itself)
    uint32_t r = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < NK; ++i) r = min(r, w[i] >= ans ? w[i] : 0xFFFFFFFFu);
    return r;
}

// m: the eroded mask (or the caller's when nothing is eroded; NULL: every voxel is foreground)
template <int K>
__global__ __launch_bounds__(AN_THREADS) void median_kernel(const float* __restrict__ a, const unsigned char* __restrict__ m,
                                                            const unsigned char* __restrict__ label, float* __restrict__ out, const MdGeom g,
                                                            unsigned long long* __restrict__ part, unsigned long long* __restrict__ results) {
    constexpr int R = K / 2, LDp = MD_TD + 2 * R, LH = MD_TH + 2 * R, LW = MD_TW + 2 * R, NL = LDp * LH * LW;
    __shared__ uint32_t keys[NL];
    __shared__ __attribute__((aligned(8))) char tail[AN_TAIL_BYTES];
    __shared__ uint32_t ext[2];
    const AnTail T = an_tail(tail);

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    int blk = blockIdx.x;
    const int tw = blk % g.tiles_w; blk /= g.tiles_w;
    const int th = blk % g.tiles_h;
    const int td = blk / g.tiles_h;
    const int d0 = td * MD_TD, h0 = th * MD_TH, w0 = tw * MD_TW;
    const int64_t vbase = b * ((int64_t)g.D * g.H * g.W);

    T.hist[tid] = 0u;
    T.hist[tid + AN_THREADS] = 0u;
    if (tid == 0) {
        ext[0] = 0xFFFFFFFFu;
        ext[1] = 0u;
    }
    __syncthreads();

    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll 4
    for (int i = tid; i < NL; i += AN_THREADS) {      // (four loads in flight: the staging is latency, not bandwidth)
        const int lw = i % LW, lh = (i / LW) % LH, ld = i / (LW * LH);
        const int d = d0 - R + ld, h = h0 - R + lh, w = w0 - R + lw;
        uint32_t key = MD_ZERO_KEY;
        if (d >= 0 && d < g.D && h >= 0 && h < g.H && w >= 0 && w < g.W) {
            const int64_t off = vbase + ((int64_t)d * g.H + h) * g.W + w;
            if (!m || m[off] != 0) key = md_key(__float_as_uint(a[off]));
        }
        keys[i] = key;
        mn = min(mn, key);
        mx = max(mx, key);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    }
    if ((tid & 63) == 0) {
        atomicMin(&ext[0], mn);
        atomicMax(&ext[1], mx);
    }
    __syncthreads();
    const uint32_t bmn = ext[0], bmx = ext[1];
    const bool flat = bmn == bmx;      // uniform over the block

    // a wave works on one 4 x 4 x 4 cube at a time (lane = z * 16 + y * 4 + x), not on a strip along W: a wave is as slow as its slowest lane, and a
    // compact cube meets the rim of a blob far less often than a 2 x 32 strip (measured on the 2 % blob field: DESIGN 7.18).  For k = 5 (rows of 36
    // words, planes of 720) the 64 reads of one window instruction fall into 64 different LDS banks; k = 3 (34, 612) has two-way conflicts.
    const int lane = tid & 63, wave = tid >> 6;
    AnAcc acc;
#pragma unroll 1
    for (int j = 0; j < MD_PER_THREAD; ++j) {
        const int cube = j * 4 + wave;      // 0..63: (cube >> 5, (cube >> 3) & 3, cube & 7) in units of 4 voxels
        const int dl = (cube >> 5) * 4 + (lane >> 4), hh = ((cube >> 3) & 3) * 4 + ((lane >> 2) & 3), wl = (cube & 7) * 4 + (lane & 3);
        const int d = d0 + dl, h = h0 + hh, w = w0 + wl;
        if (d < g.D && h < g.H && w < g.W) {
            const uint32_t key = flat ? bmn : md_select<K, LH, LW>(keys + (dl * LH + hh) * LW + wl);
            const int64_t off = vbase + ((int64_t)d * g.H + h) * g.W + w;
            const bool fg = !m || m[off] != 0;
            const float o = __uint_as_float(fg ? md_bits(key) : 0u);
            out[off] = o;
            an_account(acc, T.hist, o, (label && label[off] != 0) ? 1u : 0u, g.inv_bin, g.has_t != 0, g.t);
        }
    }
    an_block_finish(acc, T, part + (b * g.nblk + blockIdx.x) * AN_PART, results + b * AN_WORDS);
}

__global__ __launch_bounds__(256) void median_finish_kernel(const unsigned long long* __restrict__ part, int nblk, unsigned long long* __restrict__ results) {
    an_finish_body(part, nblk, results);
}

}  // namespace sa

using namespace sa;

namespace {

int64_t md_align(int64_t v) { return (v + 15) & ~(int64_t)15; }

int md_plan(const sa_median_params& P, MdGeom& g) {
    if (P.B < 1 || P.D < 1 || P.H < 1 || P.W < 1) return SA_EINVAL;
    if (P.size != 1 && P.size != 3 && P.size != 5) return SA_EINVAL;
    if (P.erosion < 0 || P.erosion > SA_MEDIAN_MAX_EROSION) return SA_EINVAL;
    if (P.erosion > 0 && !P.has_mask) return SA_EINVAL;
    if (!(P.inv_bin > 0.f) || P.inv_bin - P.inv_bin != 0.f) return SA_EINVAL;
    if (P.has_threshold && P.threshold - P.threshold != 0.f) return SA_EINVAL;
    if (P.B > 65535) return SA_EUNSUPPORTED;
    const int64_t vol = (int64_t)P.D * P.H * P.W;
    if (vol >= 0x7fffffffll) return SA_EUNSUPPORTED;
    g.D = P.D; g.H = P.H; g.W = P.W;
    g.tiles_h = (P.H + MD_TH - 1) / MD_TH;
    g.tiles_w = (P.W + MD_TW - 1) / MD_TW;
    g.nblk = (int)((int64_t)((P.D + MD_TD - 1) / MD_TD) * g.tiles_h * g.tiles_w);      // (<= vol)
    g.has_t = P.has_threshold != 0;
    g.inv_bin = P.inv_bin;
    g.t = P.threshold;
    return 0;
}

// the workspace: the blocks' partial words [B][nblk][AN_PART], then one byte volume [B][vol] per erosion buffer (one for a single step, two beyond)
int64_t md_part_bytes(const sa_median_params& P, const MdGeom& g) { return md_align((int64_t)P.B * g.nblk * AN_PART * 8); }
int64_t md_mask_bytes(const sa_median_params& P) { return md_align((int64_t)P.B * P.D * P.H * P.W); }

}  // namespace

extern "C" int64_t sa_anomaly_median_workspace_bytes(const sa_median_params* params) {
    if (!params) return SA_EINVAL;
    MdGeom g;
    const int rc = md_plan(*params, g);
    return rc ? rc : md_part_bytes(*params, g) + (params->erosion > 1 ? 2 : params->erosion) * md_mask_bytes(*params);
}

extern "C" int sa_anomaly_median(const float* a, const unsigned char* mask, const unsigned char* label, float* out, const sa_median_params* params,
                                 void* results, void* ws, void* stream) {
    if (!a || !out || !params || !results || !ws || (((uintptr_t)results) & 7u) != 0 || (((uintptr_t)ws) & 15u) != 0) return SA_EINVAL;
    if ((const float*)out == a) return SA_EINVAL;
    if ((mask != nullptr) != (params->has_mask != 0) || (label != nullptr) != (params->has_labels != 0)) return SA_EINVAL;
    MdGeom g;
    const int rc = md_plan(*params, g);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned B = (unsigned)params->B;
    const int64_t vol = (int64_t)g.D * g.H * g.W;
    unsigned long long* part = (unsigned long long*)ws;
    unsigned char* buf[2] = {(unsigned char*)ws + md_part_bytes(*params, g), (unsigned char*)ws + md_part_bytes(*params, g) + md_mask_bytes(*params)};
    if (hipMemsetAsync(results, 0, (size_t)B * AN_WORDS * 8, st) != hipSuccess) {
        g_last_error = hipGetLastError();
        return (int)g_last_error;
    }
    const unsigned char* m = mask;
    for (int s = 0; s < params->erosion; ++s) {
        SA_LAUNCH(median_erode_kernel, dim3((unsigned)((vol + 255) / 256), B), dim3(256), 0, st, m, buf[s & 1], g.D, g.H, g.W);
        SA_CHECK_LAUNCH();
        m = buf[s & 1];
    }
    const dim3 grid((unsigned)g.nblk, B), block(AN_THREADS);
    if (params->size == 5) {
        SA_LAUNCH(median_kernel<5>, grid, block, 0, st, a, m, label, out, g, part, (unsigned long long*)results);
    } else if (params->size == 3) {
        SA_LAUNCH(median_kernel<3>, grid, block, 0, st, a, m, label, out, g, part, (unsigned long long*)results);
    } else {
        SA_LAUNCH(median_kernel<1>, grid, block, 0, st, a, m, label, out, g, part, (unsigned long long*)results);
    }
    SA_CHECK_LAUNCH();
    SA_LAUNCH(median_finish_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)part, g.nblk, (unsigned long long*)results);
    SA_CHECK_LAUNCH();
    return 0;
}
