// MS-SSIM of pytorch_msssim 0.2.1 (`ms_ssim`, as the reference's MultiScaleSSIM metric calls it: src/metrics/vqvae.py) over 5-D volumes, every level on the
// stream with no host synchronisation.  Contract: per level l, with G = the 1-D window applied along D, H, W in valid mode,
//   mu_x = G(x), mu_y = G(y), s_x = G(x^2) - mu_x^2, s_y = G(y^2) - mu_y^2, s_xy = G(xy) - mu_x mu_y
//   cs = (2 s_xy + C2) / (s_x + s_y + C2), ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs, both averaged over the valid region per (b, c);
// between levels x and y go through avg_pool3d(2, 2, padding = side % 2, count_include_pad) ; the result per (b, c) is
// prod_l relu(cs_l)^w_l (l < L-1) * relu(ssim_{L-1})^w_{L-1}, and out_b[b] is its mean over channels.
//
// Structure (2.5-D blocking, as sa_baur_loss): a block owns a 16 x 16 (H x W) tile of OUTPUT voxels of one (b, c) and a run of output D planes.  Each
// input plane of the run (tile + (WS - 1) halo) goes through LDS; the five moments are filtered along W there (into a second LDS buffer), then along H
// by each thread for its own column, and the H / W-filtered planes are folded into a ring of WS accumulators in registers (slot = output plane mod WS,
// a compile-time index because the march is unrolled by WS with static_for) that is the D filter.  The ring slot that completes yields ssim / cs of one output voxel.
// The same pass writes the 2 x 2 x 2-pooled x and y of the next level: pooled voxel (k, i, j) covers input [2k - pd, 2k - pd + 1] x ... and belongs to
// the block whose output range holds its window start (the first tile / run also takes start -1, the last ones every start up to side - 2), so each
// pooled voxel is written exactly once.  Each block leaves (sum ssim, sum cs) in fp64; one block sums them per (level, b, c) in a fixed order and
// combines the levels.  No atomics, and a block never straddles volumes: a volume's result is bitwise the same alone or inside any batch.
#include <type_traits>
#include <utility>

#include "sa_common.h"

namespace sa {

constexpr int SSIM_T = 16;                 // output tile: 16 x 16 (H x W), one output column per thread
constexpr int SSIM_THREADS = SSIM_T * SSIM_T;
constexpr int SSIM_MAX_WIN = 11;
constexpr int SSIM_MAX_LEVELS = 8;
constexpr int SSIM_VOL_BLOCKS = 768;       // D is split into runs until a VOLUME has about this many blocks (>= 8 output planes per run);
                                           // the split depends on the volume's shape only, never on the batch
struct SsimParams {
    float g[SSIM_MAX_WIN];
    float c1, c2;
};

struct SsimGeom {
    int D, H, W;               // input sides of this level
    int Do, Ho, Wo;            // valid output sides
    int tiles_h, tiles_w, chunks, dch;
    int nblk;                  // blocks per volume
};

static SsimGeom ssim_geom(int D, int H, int W, int ws) {
    SsimGeom g;
    g.D = D; g.H = H; g.W = W;
    g.Do = D - ws + 1; g.Ho = H - ws + 1; g.Wo = W - ws + 1;
    g.tiles_h = (g.Ho + SSIM_T - 1) / SSIM_T;
    g.tiles_w = (g.Wo + SSIM_T - 1) / SSIM_T;
    const int tiles = g.tiles_h * g.tiles_w;
    int want = (SSIM_VOL_BLOCKS + tiles - 1) / tiles;
    const int most = (g.Do + 7) / 8;
    want = want < 1 ? 1 : (want > most ? most : want);
    g.dch = (g.Do + want - 1) / want;
    g.chunks = (g.Do + g.dch - 1) / g.dch;
    g.nblk = tiles * g.chunks;
    return g;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>) in order: the ring slots of the D filter become compile-time register indices
template <typename F, int... Rs> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Rs...>) {
    (f(std::integral_constant<int, Rs>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// [lo, hi) of the pooled indices whose window start 2 i - pad lies in this block's range [r0, r1) of output positions; the first block also owns
// start -pad, the last every start up to side - 2
__device__ __forceinline__ void pooled_range(int r0, int r1, bool first, bool last, int side, int pad, int& lo, int& hi) {
    const int rlo = first ? -pad : r0, rhi = last ? side - 1 : r1;
    lo = (rlo + pad + 1) >> 1;
    hi = (rhi + pad + 1) >> 1;
}

// One level.  x, y: [BC, D, H, W] of this level; px, py (may be null: last level): [BC, (D+1)/2, (H+1)/2, (W+1)/2]; part[(bc * nblk + blk) * 2 + {0, 1}]
template <int WS>
__global__ __launch_bounds__(SSIM_THREADS) void ms_ssim_level_kernel(const float* __restrict__ x, const float* __restrict__ y, SsimGeom g, SsimParams sp,
                                                                       float* __restrict__ px, float* __restrict__ py, double* __restrict__ part) {
    constexpr int IT = SSIM_T + WS - 1;                         // input tile side (tile + halo)
    constexpr int NLD = (IT * IT + SSIM_THREADS - 1) / SSIM_THREADS;
    constexpr int NWF = (IT * SSIM_T + SSIM_THREADS - 1) / SSIM_THREADS;
    __shared__ float xs[IT * IT], ys[IT * IT];
    __shared__ float wf[5][IT * SSIM_T];                          // W-filtered moments x, y, x^2, y^2, xy: [row][output column]
    __shared__ double red[2][SSIM_THREADS / 64];

    const int tid = threadIdx.x, tx = tid % SSIM_T, ty = tid / SSIM_T;
    const int64_t bc = blockIdx.y;
    int b = blockIdx.x;
    const int tw = b % g.tiles_w; b /= g.tiles_w;
    const int th = b % g.tiles_h;
    const int chunk = b / g.tiles_h;
    const int h0 = th * SSIM_T, w0 = tw * SSIM_T;
    const int q0 = chunk * g.dch, q1 = min(q0 + g.dch, g.Do);
    const int pend = q1 + WS - 1;                                 // input planes [q0, pend)
    const int64_t plane = (int64_t)g.H * g.W;
    const float* xv = x + bc * plane * g.D;
    const float* yv = y + bc * plane * g.D;
    const bool valid = h0 + ty < g.Ho && w0 + tx < g.Wo;

    // pooled ownership (next level)
    const bool pool = px != nullptr;
    const int pd = g.D & 1, ph = g.H & 1, pw = g.W & 1;
    const int Hp = (g.H + 1) >> 1, Wp = (g.W + 1) >> 1, Dp = (g.D + 1) >> 1;
    int klo = 0, khi = 0, ilo = 0, ihi = 0, jlo = 0, jhi = 0;
    pooled_range(q0, q1, chunk == 0, chunk == g.chunks - 1, g.D, pd, klo, khi);
    pooled_range(h0, h0 + SSIM_T, th == 0, th == g.tiles_h - 1, g.H, ph, ilo, ihi);
    pooled_range(w0, w0 + SSIM_T, tw == 0, tw == g.tiles_w - 1, g.W, pw, jlo, jhi);
    const int nj = jhi - jlo;
    const bool pcell = pool && tid < (ihi - ilo) * nj;
    const int pi = pcell ? ilo + tid / nj : 0, pj = pcell ? jlo + tid % nj : 0;
    const int pr = 2 * pi - ph - h0, pc = 2 * pj - pw - w0;      // window start relative to the LDS tile (-1 only at the volume's first row / column)
    const int64_t pbase = bc * (int64_t)Dp * Hp * Wp + (int64_t)pi * Wp + pj;
    float ppx = 0.f, ppy = 0.f;

    float nx[NLD], ny[NLD];
    auto fetch = [&](int p) {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int e = tid + k * SSIM_THREADS;
            const int r = e / IT, c = e - r * IT;
            const int hh = h0 + r, ww = w0 + c;
            const bool ok = e < IT * IT && hh < g.H && ww < g.W;
            const int64_t o = (int64_t)p * plane + (int64_t)hh * g.W + ww;
            nx[k] = ok ? xv[o] : 0.f;
            ny[k] = ok ? yv[o] : 0.f;
        }
    };

    float acc[WS][5];
#pragma unroll
    for (int s = 0; s < WS; ++s)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[s][m] = 0.f;
    double s_ssim = 0.0, s_cs = 0.0;

    fetch(q0);
    for (int base = q0; base < pend; base += WS) {
        static_for<WS>([&](auto R) {
            constexpr int r = decltype(R)::value;
            const int p = base + r;
            if (p >= pend) return;
#pragma unroll
            for (int k = 0; k < NLD; ++k) {
                const int e = tid + k * SSIM_THREADS;
                if (e < IT * IT) {
                    xs[e] = nx[k];
                    ys[e] = ny[k];
                }
            }
            __syncthreads();
            if (p + 1 < pend) fetch(p + 1);                       // in flight while this plane is filtered

            // W filter of the five moments: rows 0..IT-1, output columns 0..T-1
#pragma unroll
            for (int k = 0; k < NWF; ++k) {
                const int e = tid + k * SSIM_THREADS;
                if (e < IT * SSIM_T) {
                    const int row = e / SSIM_T, col = e % SSIM_T;
                    const float* xr = xs + row * IT + col;
                    const float* yr = ys + row * IT + col;
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
                    for (int t = 0; t < WS; ++t) {
                        const float xa = xr[t], ya = yr[t], gt = sp.g[t];
                        a0 = fmaf(gt, xa, a0);
                        a1 = fmaf(gt, ya, a1);
                        a2 = fmaf(gt, xa * xa, a2);
                        a3 = fmaf(gt, ya * ya, a3);
                        a4 = fmaf(gt, xa * ya, a4);
                    }
                    wf[0][e] = a0; wf[1][e] = a1; wf[2][e] = a2; wf[3][e] = a3; wf[4][e] = a4;
                }
            }
            // 2 x 2 pooled sums of this plane for the next level
            if (pcell) {
                float sx = 0.f, sy = 0.f;
#pragma unroll
                for (int dr = 0; dr < 2; ++dr)
#pragma unroll
                    for (int dc = 0; dc < 2; ++dc) {
                        const int rr = pr + dr, cc = pc + dc;
                        if (rr >= 0 && cc >= 0) {
                            sx += xs[rr * IT + cc];
                            sy += ys[rr * IT + cc];
                        }
                    }
                const int kk = (p + pd) >> 1;                     // the pooled plane whose window holds p
                if (((p + pd) & 1) == 0) {                       // p opens the window
                    ppx = sx; ppy = sy;
                } else {                                          // p closes it (ppx = 0 if this run did not see the opening plane)
                    if (kk >= klo && kk < khi) {
                        const int64_t o = pbase + (int64_t)kk * Hp * Wp;
                        px[o] = (ppx + sx) * 0.125f;
                        py[o] = (ppy + sy) * 0.125f;
                    }
                    ppx = 0.f; ppy = 0.f;
                }
            }
            __syncthreads();

            // H filter of this thread's column, then the D filter: plane p feeds output plane q = p - (WS-1) + k with tap WS-1-k, slot (q - q0) % WS
            float v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                float a = 0.f;
#pragma unroll
                for (int t = 0; t < WS; ++t) a = fmaf(sp.g[t], wf[m][(ty + t) * SSIM_T + tx], a);
                v[m] = a;
            }
#pragma unroll
            for (int k = 0; k < WS; ++k)
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[(r + 1 + k) % WS][m] = fmaf(sp.g[WS - 1 - k], v[m], acc[(r + 1 + k) % WS][m]);
            constexpr int done = (r + 1) % WS;                   // slot of output plane p - (WS-1): complete now
            if (p >= q0 + WS - 1) {
                if (valid) {
                    const float mx = acc[done][0], my = acc[done][1];
                    const float mx2 = mx * mx, my2 = my * my, mxy = mx * my;
                    const float sx = acc[done][2] - mx2, sy = acc[done][3] - my2, sxy = acc[done][4] - mxy;
                    const float cs = (2.f * sxy + sp.c2) / (sx + sy + sp.c2);
                    const float ss = ((2.f * mxy + sp.c1) / (mx2 + my2 + sp.c1)) * cs;
                    s_ssim += (double)ss;
                    s_cs += (double)cs;
                }
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[done][m] = 0.f;
        });
    }
    s_ssim = wave_sum_f64(s_ssim);
    s_cs = wave_sum_f64(s_cs);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = s_ssim;
        red[1][tid >> 6] = s_cs;
    }
    __syncthreads();
    if (tid < 2) part[(bc * g.nblk + blockIdx.x) * 2 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

struct SsimLevels {
    int levels;
    int nblk[SSIM_MAX_LEVELS];
    int64_t part_off[SSIM_MAX_LEVELS];     // offset (doubles) of the level's partials
    double count[SSIM_MAX_LEVELS];         // valid output voxels per volume
    float w[SSIM_MAX_LEVELS];
};

// means[(l * BC + bc) * 2 + {0, 1}] = the level's mean ssim / cs of volume bc (one wave per (l, bc), lanes in a fixed order); then
// out_b[b] = mean_c prod_l relu(.)^w_l; level_means (optional) gets the means as fp32
__global__ __launch_bounds__(256) void ms_ssim_combine_kernel(const double* __restrict__ part, SsimLevels lv, int B, int C, double* __restrict__ means,
                                                              float* __restrict__ level_means, float* __restrict__ out_b) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int BC = B * C;
    for (int pair = wave; pair < lv.levels * BC; pair += 4) {
        const int l = pair / BC, bc = pair % BC;
        const double* pp = part + lv.part_off[l] + (int64_t)bc * lv.nblk[l] * 2;
        double s0 = 0.0, s1 = 0.0;
        for (int i = lane; i < lv.nblk[l]; i += 64) {
            s0 += pp[2 * i];
            s1 += pp[2 * i + 1];
        }
        s0 = wave_sum_f64(s0);
        s1 = wave_sum_f64(s1);
        if (lane == 0) {
            const double m0 = s0 / lv.count[l], m1 = s1 / lv.count[l];
            means[pair * 2] = m0;
            means[pair * 2 + 1] = m1;
            if (level_means) {
                level_means[pair * 2] = (float)m0;
                level_means[pair * 2 + 1] = (float)m1;
            }
        }
    }
    __syncthreads();    // (means were written by this block: the barrier orders global writes and reads within a work-group)
    for (int b = tid; b < B; b += 256) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) {
            double v = 1.0;
            for (int l = 0; l < lv.levels; ++l) {
                const int bc = b * C + c;
                double m = means[(l * BC + bc) * 2 + (l == lv.levels - 1 ? 0 : 1)];
                m = m > 0.0 ? m : 0.0;
                v *= pow(m, (double)lv.w[l]);
            }
            s += v;
        }
        out_b[b] = (float)(s / C);
    }
}

}  // namespace sa

using namespace sa;

namespace {

struct SsimPlan {
    SsimGeom geom[SSIM_MAX_LEVELS];
    int64_t pool_off[SSIM_MAX_LEVELS];     // byte offset of level l's x (l >= 1); y follows at + pool_bytes[l]
    int64_t pool_bytes[SSIM_MAX_LEVELS];
    int64_t part_off, means_off, total;    // bytes
    SsimLevels lv;
};

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// SA_EINVAL for what the package refuses (even window, min(H, W) <= (w-1) * 16) and for what this kernel does not cover (w outside 3..11, a level
// side shorter than the window, side < 2, levels outside 1..8)
int ssim_plan(int B, int C, int D, int H, int W, int ws, int levels, SsimPlan& P) {
    if (B < 1 || C < 1 || D < 2 || H < 2 || W < 2) return SA_EINVAL;
    if (ws % 2 == 0 || ws < 3 || ws > SSIM_MAX_WIN || levels < 1 || levels > SSIM_MAX_LEVELS) return SA_EINVAL;
    if (!((H < W ? H : W) > (ws - 1) * 16)) return SA_EINVAL;     // pytorch_msssim's assertion: the last two sides, a fixed 2^4
    if ((int64_t)B * C > 65535) return SA_EINVAL;
    P.lv.levels = levels;
    int64_t off = 0;
    int d = D, h = H, w = W;
    int64_t parts = 0;
    for (int l = 0; l < levels; ++l) {
        if (d < ws || h < ws || w < ws) return SA_EINVAL;
        P.geom[l] = ssim_geom(d, h, w, ws);
        P.lv.nblk[l] = P.geom[l].nblk;
        P.lv.part_off[l] = parts;
        P.lv.count[l] = (double)P.geom[l].Do * P.geom[l].Ho * P.geom[l].Wo;
        parts += (int64_t)B * C * P.geom[l].nblk * 2;
        if (l > 0) {
            P.pool_bytes[l] = align256((int64_t)B * C * d * h * w * (int64_t)sizeof(float));
            P.pool_off[l] = off;
            off += 2 * P.pool_bytes[l];
        }
        d = (d + 1) / 2; h = (h + 1) / 2; w = (w + 1) / 2;
    }
    P.part_off = off;
    off += align256(parts * (int64_t)sizeof(double));
    P.means_off = off;
    off += align256((int64_t)levels * B * C * 2 * (int64_t)sizeof(double));
    P.total = off;
    return 0;
}

template <int WS>
void launch_level(const float* x, const float* y, const SsimGeom& g, const SsimParams& sp, float* px, float* py, double* part, int BC, hipStream_t st) {
    SA_LAUNCH((ms_ssim_level_kernel<WS>), dim3((unsigned)g.nblk, (unsigned)BC), dim3(SSIM_THREADS), 0, st, x, y, g, sp, px, py, part);
}

}  // namespace

extern "C" int64_t sa_ms_ssim_workspace_bytes(int B, int C, int D, int H, int W, int win_size, int levels) {
    SsimPlan P;
    const int rc = ssim_plan(B, C, D, H, W, win_size, levels, P);
    return rc ? rc : P.total;
}

extern "C" int sa_ms_ssim(const float* x, const float* y, int B, int C, int D, int H, int W, const float* win, int win_size, int levels,
                          const float* weights, float c1, float c2, float* out_b, float* level_means, void* ws, void* stream) {
    if (!x || !y || !win || !weights || !out_b || !ws) return SA_EINVAL;
    SsimPlan P;
    const int rc = ssim_plan(B, C, D, H, W, win_size, levels, P);
    if (rc) return rc;
    SsimParams sp;
    for (int t = 0; t < SSIM_MAX_WIN; ++t) sp.g[t] = t < win_size ? win[t] : 0.f;
    sp.c1 = c1;
    sp.c2 = c2;
    for (int l = 0; l < levels; ++l) P.lv.w[l] = weights[l];
    char* wsb = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)(wsb + P.part_off);
    const int BC = B * C;
    const float *cx = x, *cy = y;
    for (int l = 0; l < levels; ++l) {
        float *nx = nullptr, *ny = nullptr;
        if (l + 1 < levels) {
            nx = (float*)(wsb + P.pool_off[l + 1]);
            ny = (float*)(wsb + P.pool_off[l + 1] + P.pool_bytes[l + 1]);
        }
        double* pl = part + P.lv.part_off[l];
        switch (win_size) {
            case 3: launch_level<3>(cx, cy, P.geom[l], sp, nx, ny, pl, BC, st); break;
            case 5: launch_level<5>(cx, cy, P.geom[l], sp, nx, ny, pl, BC, st); break;
            case 7: launch_level<7>(cx, cy, P.geom[l], sp, nx, ny, pl, BC, st); break;
            case 9: launch_level<9>(cx, cy, P.geom[l], sp, nx, ny, pl, BC, st); break;
            default: launch_level<11>(cx, cy, P.geom[l], sp, nx, ny, pl, BC, st); break;
        }
        SA_CHECK_LAUNCH();
        cx = nx;
        cy = ny;
    }
    SA_LAUNCH(ms_ssim_combine_kernel, dim3(1), dim3(256), 0, st, (const double*)part, P.lv, B, C, (double*)(wsb + P.means_off), level_means, out_b);
    SA_CHECK_LAUNCH();
    return 0;
}
