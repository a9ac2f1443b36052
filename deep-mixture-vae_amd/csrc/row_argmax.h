// The arg-max of a row of scores by 16 lanes: shared by the confusion-matrix count (eval_clusters.hip) and the per-row labels
// (cluster_metrics.hip), so that both name the same cluster for every row, exact ties included.
#pragma once
#include "common.h"

namespace dmvae {

// First index of the largest of s[0 .. K): the lane walks k = lane + 16 i in ascending order (strict >: the first of
// equal values within the lane), then the 16 lanes are combined, equal values going to the smaller index.  Every lane
// of the row returns the index.  K = 0 (a row that is not there): no load, the result is not used.  NaN scores are
// not ordered: the scores must not hold any.
template <typename P>
__device__ __forceinline__ int row_argmax16(P s, int K, int lane) {
    float bv = -INFINITY;
    int bi = 1 << 30;
    if (lane < K) { bv = s[lane]; bi = lane; }
    for (int k = lane + 16; k < K; k += 16) {
        const float v = s[k];
        if (v > bv) { bv = v; bi = k; }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 16);
        const int oi = __shfl_xor(bi, o, 16);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi;
}

}  // namespace dmvae
