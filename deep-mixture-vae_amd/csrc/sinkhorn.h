// Sinkhorn divergence on the device (sinkhorn.hip): the softmin pass of the log-domain Sinkhorn iteration.  Host-side launcher.
#pragma once
#include "common.h"

namespace dmvae {

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int sinkhorn_softmin_launch(hipStream_t s, const float* X, int64_t ldx, int N, const float* Y, int64_t ldy, int M, int D, const float* g, const float* log_b,
                            float eps, const float* prev, float* out);

}  // namespace dmvae
