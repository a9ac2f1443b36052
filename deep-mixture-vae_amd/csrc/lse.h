// A running logsumexp as a (maximum f32, scaled sum f64) pair and its order-free join: shared by the all-pairs kernels that keep one per row
// in registers (mixture_density.hip, sinkhorn.hip).
#pragma once
#include <math.h>

#include "common.h"

namespace dmvae {

// a running logsumexp: sum = s * exp(m); the empty pair is (-inf, 0)
struct MdLse { float m; double s; };

__device__ __forceinline__ MdLse md_join(MdLse a, MdLse b) {
#pragma clang fp contract(off)                   // (a, b) and (b, a) give the same bits: both lanes of a butterfly step hold one value
    const float M = fmaxf(a.m, b.m);
    const bool some = M > -INFINITY;
    const double ea = (double)__expf(some ? a.m - M : 0.f), eb = (double)__expf(some ? b.m - M : 0.f);
    const double pa = a.s * ea, pb = b.s * eb;
    return MdLse{M, pa + pb};
}

}  // namespace dmvae
