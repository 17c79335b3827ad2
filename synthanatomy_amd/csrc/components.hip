// Connected components of a thresholded map, the size filter and the lesion counts: sa_components (include/synthanatomy_hip.h; this
// project's own rule, the reference has no counterpart).  Per volume, with s(v) = [a(v) >= t] and c-adjacency (|offset|_1 <= 1, 2, 3 for c = 6, 18, 26):
//   id(v) = 1 + the smallest linear index of v's component where that component has >= min_size voxels, 0 elsewhere,
// and, against an optional label volume y labelled by the same rule, TP / FP / FN of the kept mask, the lesions, the lesions with a kept voxel and the
// kept components with a class-1 voxel.
//
// A union-find over the volume in a forest `parent` (int32 per voxel, -1 on the background) in which a parent's index is never above its child's, so
// a tree's root is its smallest voxel: the canonical id, whatever the tiling, the launch order or the order of the atomics.  Five launches:
//   1. local    one block per tile of 8 x 16 x 16 voxels (one (h, w) column per thread): the tile is labelled in LDS -- every voxel starts at the first
//               voxel of its run along W (one ballot), the runs are united with the rows above and the planes behind by compare-and-swap on LDS -- and
//               parent[v] = the global index of v's tile-local root, size[v] = the voxels of the piece rooted at v (0 for every other voxel; bit 31: the
//               piece holds a class-1 voxel).  Local (d, h, w) order agrees with the global one, so the local root is the piece's smallest index.
//   2. merge    one block per tile: the voxels on the tile's faces unite with their forward neighbours (3, 9 or 13 offsets) in other tiles; pairs a
//               neighbouring lane makes are skipped and the two tile-local roots of a union are pointed at its root.
//   3. flatten  every tile-local root finds its global root, points to it, and adds its piece's size (and flag) into the root's slot: one atomic per
//               piece of a tile, not per voxel (11 000 adds to one word cost 350 us).
//   4. filter   per voxel root = parent[parent[v]], ids, and the block's partial counts; the lesion hit flags.
//   5. finish   one block per volume adds the partials in a fixed order (as anomaly_finish_kernel does).
// Both volumes (the map and, with labels, y) go through 1 to 3 in the same launches (grid.z).  No block waits for another one anywhere, and every
// word of the workspace that is read has been written by launch 1 or 4 of the same call: two calls on one workspace give the same bits.
#include "sa_common.h"

namespace sa {

constexpr int CC_TD = SA_COMPONENTS_TILE_D, CC_TH = SA_COMPONENTS_TILE_H, CC_TW = SA_COMPONENTS_TILE_W;
constexpr int CC_TILE = CC_TD * CC_TH * CC_TW;
constexpr int CC_THREADS = CC_TH * CC_TW;      // one (h, w) column of the tile per thread, a wave = four rows of 16
constexpr int CC_VPT = 8;                      // voxels per thread of the flat launches 3 and 4
constexpr int CC_CHUNK = CC_THREADS * CC_VPT;
constexpr int CC_PART = 12;                    // 64-bit words a block of launch 4 leaves in the workspace (11 used)
constexpr uint32_t CC_FLAG = 0x80000000u, CC_COUNT = 0x7fffffffu;
static_assert(CC_TW == 16 && CC_THREADS == 256, "the run start below is one 16-bit mask per row, four rows per wave");

struct CcGeom {
    int D, H, W, vol;
    int tiles_h, tiles_w, ntiles, nchunks;
    int norm;          // 1, 2, 3: the largest |offset|_1 of a neighbour
    int min_size, has_labels;
    float t;
};

// forward half of the 3 x 3 x 3 neighbourhood: offset i = 0 .. 12 in ascending (dd, dh, dw) order, (0, 0, 1) first and (1, 1, 1) last
__device__ __forceinline__ void cc_offset(int i, int& dd, int& dh, int& dw) {
    const int q = i + 14;
    dd = q / 9 - 1;
    dh = (q / 3) % 3 - 1;
    dw = q % 3 - 1;
}

// ---- the tile in LDS ----
__device__ __forceinline__ int cc_lds_find(int* lab, int x) {
    int p;
    while ((p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
    return x;
}
// lock-free: a link is made only by a compare-and-swap onto a node that is a root at that instant, and always towards the smaller index
__device__ __forceinline__ void cc_lds_union(int* lab, int a, int b) {
    for (;;) {
        a = cc_lds_find(lab, a);
        b = cc_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicCAS(lab + a, a, b);
        if (old == a) return;
        a = old;      // somebody linked a first: go on from where it points now
    }
}

struct CcTile {
    int d0, h0, w0;
};
__device__ __forceinline__ CcTile cc_tile(const CcGeom& g) {
    int blk = blockIdx.x;
    const int tw = blk % g.tiles_w; blk /= g.tiles_w;
    const int th = blk % g.tiles_h;
    return CcTile{(blk / g.tiles_h) * CC_TD, th * CC_TH, tw * CC_TW};
}

// launch 1.  parent / size: [sources][B][vol]; source 0 is the map, source 1 the label volume
__global__ __launch_bounds__(CC_THREADS) void components_local_kernel(const float* __restrict__ a, const unsigned char* __restrict__ y,
                                                                      int* __restrict__ parent, uint32_t* __restrict__ size, const CcGeom g) {
    __shared__ int lab[CC_TILE];
    __shared__ uint32_t cnt[CC_TILE];
    const int tid = threadIdx.x, wl = tid % CC_TW, hl = tid / CC_TW, lane = tid & 63;
    const int src = blockIdx.z;
    const int64_t vb = (int64_t)blockIdx.y * g.vol;
    const int64_t sb = ((int64_t)src * gridDim.y + blockIdx.y) * g.vol;
    const CcTile T = cc_tile(g);
    const int h = T.h0 + hl, w = T.w0 + wl;
    const bool col = h < g.H && w < g.W;

    uint32_t fgm = 0u, clm = 0u;      // bit k: voxel k of the column is foreground / of class 1
#pragma unroll
    for (int k = 0; k < CC_TD; ++k) {
        const bool in = col && T.d0 + k < g.D;
        bool fg = false, cl = false;
        if (in) {
            const int64_t gi = vb + ((int64_t)(T.d0 + k) * g.H + h) * g.W + w;
            if (src == 0) {
                fg = a[gi] >= g.t;      // (false for a NaN)
                cl = fg && y && y[gi] != 0;
            } else {
                fg = y[gi] != 0;
            }
        }
        fgm |= (uint32_t)fg << k;
        clm |= (uint32_t)cl << k;
        // the first voxel of this voxel's run along W: behind the highest background bit below it in its row's mask
        const uint32_t row = (uint32_t)(__ballot(fg) >> (lane & 48)) & 0xffffu;
        const uint32_t below = ~row & ((1u << wl) - 1u);
        const int start = below ? 32 - __clz(below) : 0;
        const int li = (k * CC_TH + hl) * CC_TW + wl;
        lab[li] = fg ? li - wl + start : -1;
        cnt[li] = 0u;
    }
    __syncthreads();

    // unite with the rows (dd, dh) = (0, 1), (1, -1), (1, 0), (1, 1) in front: their middle voxel alone where it is foreground (its run holds the two
    // beside it), the two diagonal ones otherwise.  (0, 0, 1) is the run itself.  A label's sign never changes, so the plain reads of it are safe.
#pragma unroll
    for (int k = 0; k < CC_TD; ++k) {
        if (!((fgm >> k) & 1u)) continue;
        const int li = (k * CC_TH + hl) * CC_TW + wl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int dd = r == 0 ? 0 : 1, dh = r == 0 ? 1 : r - 2;
            const int nrm = dd + (dh < 0 ? -dh : dh);
            const int nk = k + dd, nh = hl + dh;
            if (nrm > g.norm || nk >= CC_TD || nh < 0 || nh >= CC_TH) continue;
            const int nb = (nk * CC_TH + nh) * CC_TW + wl;
            if (lab[nb] >= 0) {
                cc_lds_union(lab, li, nb);
            } else if (nrm + 1 <= g.norm) {
                if (wl > 0 && lab[nb - 1] >= 0) cc_lds_union(lab, li, nb - 1);
                if (wl < CC_TW - 1 && lab[nb + 1] >= 0) cc_lds_union(lab, li, nb + 1);
            }
        }
    }
    __syncthreads();

    // roots, and the size of every piece: lanes of a wave that follow each other with the same root add once
    int* par = parent + sb;
#pragma unroll
    for (int k = 0; k < CC_TD; ++k) {
        const bool in = col && T.d0 + k < g.D;
        const bool fg = (fgm >> k) & 1u;
        const int li = (k * CC_TH + hl) * CC_TW + wl;
        const int r = fg ? cc_lds_find(lab, li) : -1;
        if (in) {
            int gr = -1;
            if (fg) {
                const int rk = r / (CC_TH * CC_TW), rh = (r / CC_TW) % CC_TH, rw = r % CC_TW;
                gr = ((T.d0 + rk) * g.H + (T.h0 + rh)) * g.W + (T.w0 + rw);      // (< vol < 2^31)
            }
            par[((T.d0 + k) * g.H + h) * g.W + w] = gr;
        }
        const int prev = __shfl_up(r, 1, 64);
        const bool head = lane == 0 || prev != r;
        const unsigned long long heads = __ballot(head), cls = __ballot((clm >> k) & 1u);
        if (head && r >= 0) {
            const unsigned long long above = (heads >> lane) >> 1;
            const int len = above ? __ffsll((long long)above) : 64 - lane;
            const unsigned long long run = len == 64 ? ~0ull : ((1ull << len) - 1ull) << lane;
            atomicAdd(&cnt[r], (uint32_t)len);
            if (cls & run) atomicOr(&cnt[r], CC_FLAG);
        }
    }
    __syncthreads();
    uint32_t* sz = size + sb;
#pragma unroll
    for (int k = 0; k < CC_TD; ++k)
        if (col && T.d0 + k < g.D) sz[((T.d0 + k) * g.H + h) * g.W + w] = cnt[(k * CC_TH + hl) * CC_TW + wl];
}

// ---- the forest in global memory ----
// Launch 2 reads `parent` while other blocks link roots.  A load may return an OLD value -- a line held in this CU's L1, or in the L2 of another XCD (the
// L2s are not coherent with each other) -- and that is harmless: a link is only ever made by a device-scope compare-and-swap onto a node that is a
// root at that instant, towards a smaller index, and no link is ever undone, so every value a word has held names a member of the node's final set
// (itself included).  A find over old links therefore ends at a node of the right set that may no longer be a root; the compare-and-swap, which acts
// on the word itself, then fails and returns where the node points now, a smaller index, and the loop goes on from there.  A retry happens only
// because another thread has linked, and the loop is bounded by the chain's length.  The loads are relaxed agent-scope ones (served by L2, never by an
// L1 line that nobody refreshes) to keep retries rare, not to be correct.  Nothing here stores to `parent` except device-scope atomics on the word
// itself: a plain store could sit in one L2 and be written back over a link.  Whatever needs FINAL values runs in launch 3 and later.
__device__ __forceinline__ int cc_find(int* par, int x) {
    int p;
    while ((p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}
// A shortcut, not a link: x (no root) is pointed at r, a smaller member of its own set, by a device-scope minimum on the word.  Both properties above
// hold for it -- the word only decreases and only ever names members of x's set -- and a root is never touched (no member of a root's set is below
// it).  Without it every union across tiles walks the whole chain of tile-local roots again (all foreground: 44 tiles deep).
__device__ __forceinline__ void cc_shortcut(int* par, int x, int r) {
    if (r < x && __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > r) atomicMin(par + x, r);
}
__device__ __forceinline__ void cc_union(int* par, const int a0, const int b0) {
    int a = a0, b = b0;
    for (;;) {
        a = cc_find(par, a);
        b = cc_find(par, b);
        if (a == b) break;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicCAS(par + a, a, b);      // (device scope)
        if (old == a) break;
        a = old;
    }
    cc_shortcut(par, a0, b);      // (b: the smaller root, the root of both at that instant)
    cc_shortcut(par, b0, b);
}

// launch 2: the voxels on the tile's faces and their forward neighbours outside the tile.  Most of these pairs repeat a union that a neighbour makes
// (a flat contact between two pieces is hundreds of voxel pairs with the same two tile-local roots, each costing two finds through chains of roots):
// a pair is skipped when the lane before has the same pair for the same plane and offset (that lane, or the first of such a run, makes the union), or
// when this thread's last union was the same pair.  (Measured, the whole call on a 160 x 224 x 160 volume: all foreground 1 372 -> 964 us, 2 % blobs
// with labels 263 -> 212 us; with cc_shortcut on top 442 and 213 us.)  The loops are uniform over the wave: no early exit in front of the shuffles.
__global__ __launch_bounds__(CC_THREADS) void components_merge_kernel(int* __restrict__ parent, const CcGeom g) {
    const int tid = threadIdx.x, wl = tid % CC_TW, hl = tid / CC_TW, lane = tid & 63;
    int* par = parent + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * g.vol;
    const CcTile T = cc_tile(g);
    const int h = T.h0 + hl, w = T.w0 + wl;
    const bool col = h < g.H && w < g.W;
    const bool side = hl == 0 || hl == CC_TH - 1 || wl == 0 || wl == CC_TW - 1;
    int last_p = -1, last_q = -1;
    for (int k = 0; k < CC_TD; ++k) {
        const int d = T.d0 + k;
        int p = -1;
        if (col && d < g.D && (side || k == CC_TD - 1)) p = par[(d * g.H + h) * g.W + w];      // (its sign is the same in every copy: launch 1 wrote it)
        if (!__any(p >= 0)) continue;      // (the whole wave)
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            int dd, dh, dw;
            cc_offset(i, dd, dh, dw);
            if ((dh < 0 ? -dh : dh) + (dw < 0 ? -dw : dw) + dd > g.norm) continue;      // (the whole grid)
            const int nk = k + dd, nh = hl + dh, nw = wl + dw;
            const int zd = d + dd, zh = h + dh, zw = w + dw;
            int q = -1;
            if (p >= 0 && !(nk < CC_TD && nh >= 0 && nh < CC_TH && nw >= 0 && nw < CC_TW)      // (inside the tile: launch 1)
                && zd < g.D && zh >= 0 && zh < g.H && zw >= 0 && zw < g.W)
                q = par[(zd * g.H + zh) * g.W + zw];
            const int pq = q >= 0 ? p : -1;
            const bool same = __shfl_up(pq, 1, 64) == pq && __shfl_up(q, 1, 64) == q && lane > 0;
            if (q >= 0 && !same && !(last_p == p && last_q == q)) {
                cc_union(par, p, q);      // (p and q: members of the two voxels' sets)
                last_p = p;
                last_q = q;
            }
        }
    }
}

// launch 3: final values now.  A tile-local root v (size[v] != 0) points to its root and hands its piece over.  Other threads may walk through v while
// it is rewritten: both values are ancestors of v.
__global__ __launch_bounds__(CC_THREADS) void components_flatten_kernel(int* __restrict__ parent, uint32_t* __restrict__ size, const CcGeom g) {
    const int64_t sb = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * g.vol;
    int* par = parent + sb;
    uint32_t* sz = size + sb;
#pragma unroll
    for (int j = 0; j < CC_VPT; ++j) {
        const int64_t v64 = (int64_t)blockIdx.x * CC_CHUNK + j * CC_THREADS + threadIdx.x;
        if (v64 >= g.vol) break;
        const int v = (int)v64;
        const uint32_t s = sz[v];
        if (!(s & CC_COUNT)) continue;
        int r = v, p;
        while ((p = par[r]) != r) r = p;
        if (r == v) continue;
        par[v] = r;
        atomicAdd(&sz[r], s & CC_COUNT);      // (the counts of a volume stay below 2^31: no carry into the flag)
        if (s & CC_FLAG) atomicOr(&sz[r], CC_FLAG);
    }
}

__device__ __forceinline__ uint32_t cc_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t cc_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// launch 4.  counts: 0 components, 1 kept, 2 foreground voxels, 3 kept voxels, 4 largest (a maximum), 5 TP, 6 FP, 7 FN, 8 lesions, 9 lesions detected,
// 10 kept components with a class-1 voxel
__global__ __launch_bounds__(CC_THREADS) void components_filter_kernel(const int* __restrict__ parent, const uint32_t* __restrict__ size,
                                                                       const int* __restrict__ parent_y, uint32_t* __restrict__ size_y,
                                                                       const unsigned char* __restrict__ y, int* __restrict__ ids,
                                                                       unsigned long long* __restrict__ part, const CcGeom g) {
    __shared__ uint32_t red[11][4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t vb = (int64_t)blockIdx.y * g.vol;
    const int* par = parent + vb;
    const uint32_t* sz = size + vb;
    uint32_t c[11];
#pragma unroll
    for (int q = 0; q < 11; ++q) c[q] = 0u;
#pragma unroll
    for (int j = 0; j < CC_VPT; ++j) {
        const int64_t v64 = (int64_t)blockIdx.x * CC_CHUNK + j * CC_THREADS + tid;
        const bool in = v64 < g.vol;
        const int v = (int)v64;
        const int p = in ? par[v] : -1;
        bool kept = false;
        int r = -1;
        if (p >= 0) {
            r = par[p];      // (p is a tile-local root: launch 3 pointed it at the root)
            const uint32_t s = sz[r], n = s & CC_COUNT;
            kept = n >= (uint32_t)g.min_size;
            c[2] += 1u;
            c[3] += kept;
            if (r == v) {
                c[0] += 1u;
                c[1] += kept;
                c[4] = n > c[4] ? n : c[4];
                c[10] += kept && (s & CC_FLAG);
            }
        }
        if (in) ids[vb + v] = kept ? r + 1 : 0;
        if (g.has_labels) {
            const bool cl = in && y[vb + v] != 0;
            c[5] += kept && cl;
            c[6] += kept && !cl;
            c[7] += !kept && cl;
            int key = -1;
            if (cl) {
                const int ry = parent_y[vb + parent_y[vb + v]];
                c[8] += ry == v;
                if (kept) key = ry;
            }
            // the lesion's hit flag: once per run of lanes with the same lesion, and only while it still looks clear (an old copy costs one more
            // atomic); the thread whose atomic finds it clear is the one that counts the lesion
            const int prev = __shfl_up(key, 1, 64);
            if (key >= 0 && (lane == 0 || prev != key)) {
                uint32_t* f = size_y + vb + key;
                if (!(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & CC_FLAG)) c[9] += !(atomicOr(f, CC_FLAG) & CC_FLAG);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 11; ++q) c[q] = q == 4 ? cc_wave_max(c[q]) : cc_wave_sum(c[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 11; ++q) red[q][tid >> 6] = c[q];
    }
    __syncthreads();
    if (tid < CC_PART) {
        unsigned long long v = 0ull;
        if (tid == 4) {
            for (int i = 0; i < 4; ++i) v = red[4][i] > v ? red[4][i] : v;
        } else if (tid < 11) {
            v = (unsigned long long)red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
        }
        part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * CC_PART + tid] = v;
    }
}

// launch 5: one block per volume, lanes and waves in a fixed order
__global__ __launch_bounds__(256) void components_finish_kernel(const unsigned long long* __restrict__ part, int nblk, long long* __restrict__ results) {
    __shared__ unsigned long long red[11][4];
    const int tid = threadIdx.x;
    const unsigned long long* pp = part + (int64_t)blockIdx.x * nblk * CC_PART;
    unsigned long long c[11];
#pragma unroll
    for (int q = 0; q < 11; ++q) c[q] = 0ull;
    for (int i = tid; i < nblk; i += 256) {
#pragma unroll
        for (int q = 0; q < 11; ++q) {
            const unsigned long long v = pp[(int64_t)i * CC_PART + q];
            c[q] = q == 4 ? (v > c[q] ? v : c[q]) : c[q] + v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 11; ++q) {
            const unsigned long long v = __shfl_xor(c[q], o, 64);
            c[q] = q == 4 ? (v > c[q] ? v : c[q]) : c[q] + v;
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 11; ++q) red[q][tid >> 6] = c[q];
    }
    __syncthreads();
    if (tid < SA_COMPONENTS_RESULT_WORDS) {
        unsigned long long v = 0ull;
        if (tid == 4) {
            for (int i = 0; i < 4; ++i) v = red[4][i] > v ? red[4][i] : v;
        } else if (tid < 11) {
            v = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
        }
        results[(int64_t)blockIdx.x * SA_COMPONENTS_RESULT_WORDS + tid] = (long long)v;
    }
}

}  // namespace sa

using namespace sa;

namespace {

int64_t cc_align(int64_t v) { return (v + 15) & ~(int64_t)15; }

int cc_plan(const sa_components_params& P, CcGeom& g) {
    if (P.B < 1 || P.D < 1 || P.H < 1 || P.W < 1) return SA_EINVAL;
    if (P.connectivity != 6 && P.connectivity != 18 && P.connectivity != 26) return SA_EINVAL;
    if (P.min_size < 1) return SA_EINVAL;
    if (P.threshold - P.threshold != 0.f) return SA_EINVAL;
    const int64_t vol = (int64_t)P.D * P.H * P.W;
    if (vol >= 0x7fffffffll) return SA_EINVAL;
    if (P.B > 65535) return SA_EUNSUPPORTED;
    g.D = P.D; g.H = P.H; g.W = P.W;
    g.vol = (int)vol;
    g.tiles_h = (P.H + CC_TH - 1) / CC_TH;
    g.tiles_w = (P.W + CC_TW - 1) / CC_TW;
    g.ntiles = (int)((int64_t)((P.D + CC_TD - 1) / CC_TD) * g.tiles_h * g.tiles_w);      // (<= vol)
    g.nchunks = (int)((vol + CC_CHUNK - 1) / CC_CHUNK);
    g.norm = P.connectivity == 6 ? 1 : P.connectivity == 18 ? 2 : 3;
    g.min_size = P.min_size;
    g.has_labels = P.has_labels != 0;
    g.t = P.threshold;
    return 0;
}

// the workspace: parent [sources][B][vol] int32, size [sources][B][vol] uint32, the partial counts [B][nchunks][CC_PART] 64-bit words
int64_t cc_forest_bytes(const sa_components_params& P, const CcGeom& g) { return cc_align((int64_t)(g.has_labels ? 2 : 1) * P.B * g.vol * 4); }

}  // namespace

extern "C" int64_t sa_components_workspace_bytes(const sa_components_params* params) {
    if (!params) return SA_EINVAL;
    CcGeom g;
    const int rc = cc_plan(*params, g);
    return rc ? rc : 2 * cc_forest_bytes(*params, g) + (int64_t)params->B * g.nchunks * CC_PART * 8;
}

extern "C" int sa_components(const float* a, const unsigned char* label, int32_t* ids_out, const sa_components_params* params, void* results, void* ws,
                             void* stream) {
    if (!a || !ids_out || !params || !results || !ws || (((uintptr_t)results) & 7u) != 0 || (((uintptr_t)ws) & 15u) != 0) return SA_EINVAL;
    if ((label != nullptr) != (params->has_labels != 0)) return SA_EINVAL;
    CcGeom g;
    const int rc = cc_plan(*params, g);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned B = (unsigned)params->B, S = g.has_labels ? 2u : 1u;
    const int64_t fb = cc_forest_bytes(*params, g);
    int* parent = (int*)ws;
    uint32_t* size = (uint32_t*)((char*)ws + fb);
    unsigned long long* part = (unsigned long long*)((char*)ws + 2 * fb);
    const int64_t src1 = (int64_t)B * g.vol;      // the label volume's forest
    SA_LAUNCH(components_local_kernel, dim3((unsigned)g.ntiles, B, S), dim3(CC_THREADS), 0, st, a, label, parent, size, g);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(components_merge_kernel, dim3((unsigned)g.ntiles, B, S), dim3(CC_THREADS), 0, st, parent, g);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(components_flatten_kernel, dim3((unsigned)g.nchunks, B, S), dim3(CC_THREADS), 0, st, parent, size, g);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(components_filter_kernel, dim3((unsigned)g.nchunks, B), dim3(CC_THREADS), 0, st, (const int*)parent, (const uint32_t*)size,
              (const int*)(g.has_labels ? parent + src1 : nullptr), g.has_labels ? size + src1 : nullptr, label, ids_out, part, g);
    SA_CHECK_LAUNCH();
    SA_LAUNCH(components_finish_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)part, g.nchunks, (long long*)results);
    SA_CHECK_LAUNCH();
    return 0;
}
