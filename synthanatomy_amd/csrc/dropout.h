// Counter-based dropout keep decisions (performer_pytorch 1.0.11 ff_dropout / attn_dropout, reference run_transformer.py:83-84): nn.Dropout(p) keeps an element
// with probability 1 - p and scales the kept ones by 1 / (1 - p).  The decision is a pure function of (seed, site, element index), so the backward pass
// regenerates the forward's mask instead of storing it.
//
// Engine: Philox4x32-10 (Salmon et al., SC'11; the Random123 / rocRAND constants), one call = four 32-bit words = four decisions:
//   counter = { lo32(e >> 2), hi32(e >> 2), site, 0 },  key = { lo32(seed), hi32(seed) },  word = output[e & 3]
//   keep(e) = word >= thr,  thr = min(floor(p * 2^32), 2^32 - 1)  (thr = 0 keeps everything),  scale = fp32(1 / (1 - p))
// Element index e:
//   dense sites (FF hidden h, attention output F) of a [rows, cols] row-major tensor:  e = row * cols + col
//   local-window probabilities P[b, h, i, j] of sa_local_attn_*_dropout:                 e = ((b * L + h) * N + i) * N + j
// `site` separates the layers and the sites of one forward (the Performer uses 4 * layer + {0: FF hidden, 1: attention output, 2: local probabilities}).
#pragma once
#include <algorithm>
#include <cmath>

#include "sa_common.h"

namespace sa {

struct DropParams {
    uint32_t k0, k1, site, thr;
    float scale;
};

inline DropParams make_drop(float p, uint64_t seed, uint32_t site) {
    DropParams d;
    d.k0 = (uint32_t)seed;
    d.k1 = (uint32_t)(seed >> 32);
    d.site = site;
    const double t = std::floor((double)p * 4294967296.0);
    d.thr = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
    d.scale = (float)(1.0 / (1.0 - (double)p));
    return d;
}

struct Philox4 {
    uint32_t v[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the four words of elements 4 q .. 4 q + 3
__host__ __device__ __forceinline__ Philox4 drop_words4(const DropParams& d, uint64_t q) {
    return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), d.site, 0u, d.k0, d.k1);
}

__host__ __device__ __forceinline__ uint32_t drop_word(const Philox4& w, uint32_t k) { return k == 0 ? w.v[0] : k == 1 ? w.v[1] : k == 2 ? w.v[2] : w.v[3]; }

// keep / (1 - p) or 0 for element e
__host__ __device__ __forceinline__ float drop_factor(const DropParams& d, uint64_t e) {
    return drop_word(drop_words4(d, e >> 2), (uint32_t)e & 3u) >= d.thr ? d.scale : 0.f;
}

// the factors of the four consecutive elements e0 .. e0 + 3 (one Philox call when e0 is a multiple of 4, two otherwise)
__device__ __forceinline__ void drop_factors4(const DropParams& d, uint64_t e0, float (&f)[4]) {
    const uint32_t s = (uint32_t)e0 & 3u;
    const Philox4 a = drop_words4(d, e0 >> 2);
    if (s == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) f[r] = a.v[r] >= d.thr ? d.scale : 0.f;
        return;
    }
    const Philox4 b = drop_words4(d, (e0 >> 2) + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t k = s + r;
        f[r] = (k < 4 ? drop_word(a, k) : drop_word(b, k - 4)) >= d.thr ? d.scale : 0.f;
    }
}

}  // namespace sa
