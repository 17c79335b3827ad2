// BaurLoss of the reference (src/losses/vqvae/vqvae.py:74-186, --loss=baur): L1 + L2 + gdl_factor * the gradient-difference loss, and
// d loss / d pred, in one pass over pred and target.  Notation (e_a = unit step along axis a of [D, H, W]; I = interior {1..D-2} x {1..H-2} x {1..W-2}):
//   gy_a(i) = y(i - e_a) - y(i), gp_a(i) = p(i - e_a) - p(i), t_a(i) = | |gy_a| - |gp_a| |, sigma_a(i) = sign(|gy_a| - |gp_a|) * sign(gp_a)
//   sums: S1 = sum |p - y|, S2 = sum (p - y)^2 over every voxel; S3 = sum_{i in I} t_z + t_y + t_x
//   grad(j) = sign(p - y) * cn + 2 (p - y) * cn + cm * sum_a ([j in I] sigma_a(j) - [j + e_a in I] sigma_a(j + e_a))     (sign(0) = 0 everywhere)
// cn = gscale / n and cm = gscale * gdl_factor / m (reduction "mean"; gscale and gscale * gdl_factor for "sum").
//
// Structure (2.5-D blocking): a block owns a 32 x 32 (H x W) tile of one (b, c) volume and a run of consecutive D planes.  Each thread keeps one
// float4 along W of planes d and d + 1 in registers (the D neighbours; the D term of plane d was computed at plane d - 1 and is carried), and the
// current plane goes through LDS with a one-voxel H / W halo (the H and W neighbours).  Each t / sigma pair is evaluated once on the D and W axes
// and twice on H.  Plane d + 2 and the halo of plane d + 1 are in flight while plane d is computed.  Every block leaves one (S1, S2, S3)
// triple; a single block then sums them in a fixed order, so the sums and the gradient are bitwise reproducible (no atomics).
#include "sa_common.h"

namespace sa {

constexpr int BAUR_TW = 32, BAUR_TH = 32;      // tile: 8 float4 columns x 32 rows = 256 threads, one float4 each
constexpr int BAUR_LS = BAUR_TW + 8;           // LDS row: left halo at column 3, tile at 4..35 (16-B aligned), right halo at 36
constexpr int BAUR_LR = BAUR_TH + 2;           // LDS rows: halo row above, 32 tile rows, halo row below
constexpr int BAUR_TARGET_BLOCKS = 2048;       // D is split into runs until about this many blocks exist (>= 4 planes per run)

struct BaurGeom {
    int tiles_w, tiles_h, chunks, dch;
    int64_t nblk;
};

static BaurGeom baur_geom(int64_t BC, int D, int H, int W) {
    BaurGeom g;
    g.tiles_w = (W + BAUR_TW - 1) / BAUR_TW;
    g.tiles_h = (H + BAUR_TH - 1) / BAUR_TH;
    const int64_t tiles = BC * g.tiles_w * g.tiles_h;
    int64_t want = (BAUR_TARGET_BLOCKS + tiles - 1) / tiles;
    const int64_t most = (D + 3) / 4;
    want = want < 1 ? 1 : (want > most ? most : want);
    g.dch = (int)((D + want - 1) / want);
    g.chunks = (D + g.dch - 1) / g.dch;
    g.nblk = tiles * g.chunks;
    return g;
}

__device__ __forceinline__ float sgnf(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// t = | |gy| - |gp| | and sigma = sign(|gy| - |gp|) * sign(gp)
__device__ __forceinline__ void gdl_term(float gy, float gp, float& t, float& s) {
    const float a = fabsf(gy) - fabsf(gp);
    t = fabsf(a);
    s = sgnf(a) * sgnf(gp);
}
__device__ __forceinline__ float gdl_sigma(float gy, float gp) { return sgnf(fabsf(gy) - fabsf(gp)) * sgnf(gp); }

// four consecutive voxels of one row starting at column w (VEC: one aligned float4, W % 4 == 0); columns >= W and invalid rows read as 0
template <bool VEC> __device__ __forceinline__ float4 load4(const float* __restrict__ src, int64_t row, int w, int W, bool ok) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok) return v;
    if (VEC) {
        if (w < W) v = *reinterpret_cast<const float4*>(src + row + w);
    } else {
        if (w < W) v.x = src[row + w];
        if (w + 1 < W) v.y = src[row + w + 1];
        if (w + 2 < W) v.z = src[row + w + 2];
        if (w + 3 < W) v.w = src[row + w + 3];
    }
    return v;
}

template <bool VEC> __device__ __forceinline__ void store4(float* __restrict__ dst, int64_t row, int w, int W, const float (&g)[4]) {
    if (VEC) {
        if (w < W) *reinterpret_cast<float4*>(dst + row + w) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w + k < W) dst[row + w + k] = g[k];
    }
}

__device__ __forceinline__ void f4_to(const float4 v, float (&a)[4]) { a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }

// One block: tile (bc, th, tw), planes [d0, d1).  ws[k * nblk + block] = the block's partial S1 / S2 / S3 (k = 0, 1, 2).
template <bool VEC, bool GDL>
__global__ __launch_bounds__(256) void baur_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target, int D, int H, int W,
                                                        BaurGeom g, float cn, float cm, float* __restrict__ grad, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float lds[2][2][BAUR_LR * BAUR_LS];   // [buffer][p | y][row * BAUR_LS + column]
    __shared__ float red[3][4];
    const int tid = threadIdx.x, tx = tid & 7, ty = tid >> 3;
    const uint32_t bid = xcd_remap(blockIdx.x, (uint32_t)g.nblk);   // consecutive D runs of one tile share their edge planes: keep them on one L2
    int64_t b = bid;
    const int chunk = (int)(b % g.chunks); b /= g.chunks;
    const int tw = (int)(b % g.tiles_w); b /= g.tiles_w;
    const int th = (int)(b % g.tiles_h);
    const int64_t bc = b / g.tiles_h;
    const int d0 = chunk * g.dch, d1 = min(d0 + g.dch, D);
    const int h0 = th * BAUR_TH, w0 = tw * BAUR_TW;
    const int h = h0 + ty, w = w0 + 4 * tx;
    const int64_t plane = (int64_t)H * W;
    const int64_t vbase = bc * plane * D;
    const bool hok = h < H;
    auto row_of = [&](int d, int hh) { return vbase + (int64_t)d * plane + (int64_t)hh * W; };

    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (!GDL) {
        for (int d = d0; d < d1; ++d) {
            const int64_t r = row_of(d, h);
            float pc[4], yc[4], gr[4];
            f4_to(load4<VEC>(pred, r, w, W, hok), pc);
            f4_to(load4<VEC>(target, r, w, W, hok), yc);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dv = pc[k] - yc[k];     // (0 outside the volume)
                s1 += fabsf(dv);
                s2 += dv * dv;
                gr[k] = sgnf(dv) * cn + (2.f * dv) * cn;
            }
            if (grad && hok) store4<VEC>(grad, r, w, W, gr);
        }
    } else {
        // halo duties for the NEXT plane: threads 0..15 the rows above / below the tile (float4; 0..7 pred, 8..15 target, even / odd = above / below),
        // 64..127 the columns left / right of the tile for pred, 128..191 for target (scalars)
        const bool row_halo = tid < 16, col_halo = tid >= 64 && tid < 192;
        const int rh_src = (tid >> 3) & 1;                                  // row halo: 0 pred, 1 target
        const int rh_x = tid & 7;                                           // row halo: float4 column
        const int ch_src = (tid - 64) >> 6, ch_k = (tid - 64) & 63;         // column halo: 0 pred / 1 target, index
        const int ch_side = ch_k >> 5, ch_r = ch_k & 31;                    // 0 left / 1 right, tile row
        const float* rh_ptr = rh_src ? target : pred;
        const float* ch_ptr = ch_src ? target : pred;
        // a row-halo thread loads BOTH rows (above and below) of its float4 column
        auto halo_rows = [&](int d, float4& above, float4& below) {
            above = load4<VEC>(rh_ptr, row_of(d, h0 - 1), w0 + 4 * rh_x, W, h0 >= 1);
            below = load4<VEC>(rh_ptr, row_of(d, h0 + BAUR_TH), w0 + 4 * rh_x, W, h0 + BAUR_TH < H);
        };
        auto halo_col = [&](int d) {
            const int hh = h0 + ch_r, ww = ch_side ? w0 + BAUR_TW : w0 - 1;
            return (hh < H && ww >= 0 && ww < W) ? ch_ptr[row_of(d, hh) + ww] : 0.f;
        };

        float pp[4], yp[4], pc[4], yc[4], pn[4], yn[4];
        f4_to(load4<VEC>(pred, d0 >= 1 ? row_of(d0 - 1, h) : 0, w, W, hok && d0 >= 1), pp);
        f4_to(load4<VEC>(target, d0 >= 1 ? row_of(d0 - 1, h) : 0, w, W, hok && d0 >= 1), yp);
        f4_to(load4<VEC>(pred, row_of(d0, h), w, W, hok), pc);
        f4_to(load4<VEC>(target, row_of(d0, h), w, W, hok), yc);
        f4_to(load4<VEC>(pred, d0 + 1 < D ? row_of(d0 + 1, h) : 0, w, W, hok && d0 + 1 < D), pn);
        f4_to(load4<VEC>(target, d0 + 1 < D ? row_of(d0 + 1, h) : 0, w, W, hok && d0 + 1 < D), yn);
        // the D term of plane d is the "j + e_z" term of plane d - 1: computed once and carried along the march
        float tzc[4], szc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) gdl_term(yp[k] - yc[k], pp[k] - pc[k], tzc[k], szc[k]);
        float4 ha = make_float4(0.f, 0.f, 0.f, 0.f), hb = ha;
        float hc = 0.f;
        if (row_halo) halo_rows(d0, ha, hb);
        if (col_halo) hc = halo_col(d0);

        const bool hin = h >= 1 && h <= H - 2, hin1 = h + 1 <= H - 2;       // [h in 1..H-2], [h + 1 in 1..H-2]
        for (int d = d0, it = 0; d < d1; ++d, ++it) {
            // in flight during this plane: plane d + 2 (the next iteration's d + 1) and the halo of plane d + 1
            const bool more = d + 1 < d1;
            float4 nnp = make_float4(0.f, 0.f, 0.f, 0.f), nny = nnp, nha = nnp, nhb = nnp;
            float nhc = 0.f;
            if (more) {
                const bool ok2 = hok && d + 2 < D;
                nnp = load4<VEC>(pred, ok2 ? row_of(d + 2, h) : 0, w, W, ok2);
                nny = load4<VEC>(target, ok2 ? row_of(d + 2, h) : 0, w, W, ok2);
                if (row_halo) halo_rows(d + 1, nha, nhb);
                if (col_halo) nhc = halo_col(d + 1);
            }
            float* lp = lds[it & 1][0];
            float* ly = lds[it & 1][1];
            const int c0 = (ty + 1) * BAUR_LS + 4 + 4 * tx;
            *reinterpret_cast<float4*>(lp + c0) = make_float4(pc[0], pc[1], pc[2], pc[3]);
            *reinterpret_cast<float4*>(ly + c0) = make_float4(yc[0], yc[1], yc[2], yc[3]);
            if (row_halo) {
                float* l = rh_src ? ly : lp;
                *reinterpret_cast<float4*>(l + 4 + 4 * rh_x) = ha;
                *reinterpret_cast<float4*>(l + (BAUR_TH + 1) * BAUR_LS + 4 + 4 * rh_x) = hb;
            }
            if (col_halo) (ch_src ? ly : lp)[(ch_r + 1) * BAUR_LS + (ch_side ? 4 + BAUR_TW : 3)] = hc;
            __syncthreads();       // (double-buffered: the next plane's writes go to the other buffer, whose readers have all passed this barrier)

            const float4 pu4 = *reinterpret_cast<const float4*>(lp + c0 - BAUR_LS), yu4 = *reinterpret_cast<const float4*>(ly + c0 - BAUR_LS);
            const float4 pd4 = *reinterpret_cast<const float4*>(lp + c0 + BAUR_LS), yd4 = *reinterpret_cast<const float4*>(ly + c0 + BAUR_LS);
            float pu[4], yu[4], pd[4], yd[4];
            f4_to(pu4, pu); f4_to(yu4, yu); f4_to(pd4, pd); f4_to(yd4, yd);
            const float pl = lp[c0 - 1], yl = ly[c0 - 1], pr = lp[c0 + 4], yr = ly[c0 + 4];

            const bool din = d >= 1 && d <= D - 2, din1 = d + 1 <= D - 2;
            // W terms at columns w .. w + 4: column w + k + 1's own term is column w + k's "j + e_x" term
            float txs[5], sxs[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float pm = k == 0 ? pl : pc[k - 1], ym = k == 0 ? yl : yc[k - 1];
                const float p0 = k == 4 ? pr : pc[k], y0 = k == 4 ? yr : yc[k];
                gdl_term(ym - y0, pm - p0, txs[k], sxs[k]);
            }
            float gr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int wk = w + k;
                const bool valid = hok && wk < W;
                const bool win = wk >= 1 && wk <= W - 2, win1 = wk + 1 <= W - 2;
                const float dv = pc[k] - yc[k];
                float tyy, sy, tzn, szn;
                gdl_term(yu[k] - yc[k], pu[k] - pc[k], tyy, sy);
                gdl_term(yc[k] - yn[k], pc[k] - pn[k], tzn, szn);
                const bool interior = valid && din && hin && win;
                float S = 0.f;
                if (interior) {
                    s3 += (tzc[k] + tyy) + txs[k];
                    S = (szc[k] + sy) + sxs[k];
                }
                if (din1 && hin && win) S -= szn;                                             // j + e_z in I
                if (din && hin1 && win) S -= gdl_sigma(yc[k] - yd[k], pc[k] - pd[k]);       // j + e_y in I
                if (din && hin && win1) S -= sxs[k + 1];                                      // j + e_x in I
                tzc[k] = tzn;
                szc[k] = szn;
                if (valid) {
                    s1 += fabsf(dv);
                    s2 += dv * dv;
                }
                gr[k] = (sgnf(dv) * cn + (2.f * dv) * cn) + S * cm;
            }
            if (grad && hok) store4<VEC>(grad, row_of(d, h), w, W, gr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pc[k] = pn[k]; yc[k] = yn[k];
            }
            f4_to(nnp, pn);
            f4_to(nny, yn);
            ha = nha; hb = nhb; hc = nhc;
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = s1;
        red[1][tid >> 6] = s2;
        red[2][tid >> 6] = s3;
    }
    __syncthreads();
    if (tid < 3) ws[(int64_t)tid * g.nblk + bid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// sums3[k] = sum over blocks of ws[k * nblk + block], in fp64 and a fixed order (one block of 256 threads)
__global__ __launch_bounds__(256) void baur_sum_kernel(const float* __restrict__ ws, int64_t nblk, float* __restrict__ sums3) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        for (int64_t i = tid; i < nblk; i += 256) s += (double)ws[k * nblk + i];
        red[k][tid] = s;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
        __syncthreads();
    }
    if (tid < 3) sums3[tid] = (float)red[tid][0];
}

}  // namespace sa

using namespace sa;

static bool baur_shape_ok(int64_t BC, int D, int H, int W) { return BC >= 1 && D >= 3 && H >= 3 && W >= 3; }

extern "C" int64_t sa_baur_loss_workspace_bytes(int64_t BC, int D, int H, int W) {
    if (!baur_shape_ok(BC, D, H, W)) return SA_EINVAL;
    return 3 * baur_geom(BC, D, H, W).nblk * (int64_t)sizeof(float);
}

extern "C" int sa_baur_loss(const float* pred, const float* target, int64_t BC, int D, int H, int W, float gdl_factor, int reduction_sum, float gscale,
                            float* sums3, float* grad, float* ws, void* stream) {
    if (!pred || !target || !sums3 || !ws || !baur_shape_ok(BC, D, H, W)) return SA_EINVAL;
    const BaurGeom g = baur_geom(BC, D, H, W);
    if (g.nblk > 0x7fffffff) return SA_EUNSUPPORTED;
    const double n = (double)BC * D * H * W, m = (double)BC * (D - 2) * (H - 2) * (W - 2);
    const float cn = reduction_sum ? gscale : (float)((double)gscale / n);
    const float cm = reduction_sum ? (float)((double)gscale * gdl_factor) : (float)((double)gscale * gdl_factor / m);
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    const bool vec = W % 4 == 0 && al16(pred) && al16(target) && (!grad || al16(grad));
    const bool gdl = gdl_factor != 0.f;     // factor 0: the GDL term and its gradient are 0 * (finite) -- skip the stencil
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk), blk(256);
    if (vec && gdl) SA_LAUNCH((baur_loss_kernel<true, true>), grid, blk, 0, st, pred, target, D, H, W, g, cn, cm, grad, ws);
    else if (vec) SA_LAUNCH((baur_loss_kernel<true, false>), grid, blk, 0, st, pred, target, D, H, W, g, cn, cm, grad, ws);
    else if (gdl) SA_LAUNCH((baur_loss_kernel<false, true>), grid, blk, 0, st, pred, target, D, H, W, g, cn, cm, grad, ws);
    else SA_LAUNCH((baur_loss_kernel<false, false>), grid, blk, 0, st, pred, target, D, H, W, g, cn, cm, grad, ws);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(baur_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, g.nblk, sums3);
    SA_CHECK_LAUNCH();
    return 0;
}
