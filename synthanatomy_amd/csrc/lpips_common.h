// What the two LPIPS translation units (csrc/lpips.hip, csrc/lpips_squeeze.hip) share on the host side: the 2.5D slice view and the extent guard.
#pragma once
#include "sa_common.h"

namespace sa {

// a 2.5D view of the volume [B, D, H, W]: slice id = b * n + a (a along the view's axis), pixel (i, j) of the slice at b * sb + a * sa + i * si + j * sj.
// No permuted copy of the volume exists: the first-layer kernels and their adjoints read and write the fp32 volume through these strides.
struct LpView {
    int32_t n, h, w;
    int64_t sb, sa, si, sj;
};
static inline bool make_view(int view, int D, int H, int W, LpView& v) {
    v.sb = (int64_t)D * H * W;
    if (view == 0) { v.n = D; v.h = H; v.w = W; v.sa = (int64_t)H * W; v.si = W; v.sj = 1; }           // permute (0, 2, 1, 3, 4): [B D, 1, H, W]
    else if (view == 1) { v.n = H; v.h = D; v.w = W; v.sa = W; v.si = (int64_t)H * W; v.sj = 1; }      // permute (0, 3, 1, 2, 4): [B H, 1, D, W]
    else if (view == 2) { v.n = W; v.h = D; v.w = H; v.sa = 1; v.si = (int64_t)H * W; v.sj = W; }      // permute (0, 4, 1, 2, 3): [B W, 1, D, H]
    else return false;
    return true;
}

// an element count that a 32-bit thread index (256 per block) can span
static inline bool lp_ok(int64_t v) { return v > 0 && v < (1ll << 31) - 256; }

// one launch per compute dtype; SA_LAUNCH keeps the kernel's name (with its template argument) for sa_kernel_log_*
#define LP_LAUNCH_T(dtype, kern, ...)                            \
    do {                                                         \
        if ((dtype) == SA_F32) SA_LAUNCH(kern<float>, __VA_ARGS__); \
        else SA_LAUNCH(kern<bf16_t>, __VA_ARGS__);               \
    } while (0)

}  // namespace sa
