// Sample quality on the device (prdc.hip): the all-pairs counts behind precision, recall, density and coverage.  Host-side launcher.
#pragma once
#include "common.h"

namespace dmvae {

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int prdc_counts_launch(hipStream_t s, const float* R, int64_t ldr, int N, const float* F, int64_t ldf, int M, int D, const float* rR2, const float* rF2,
                       int32_t* fake_in_real, int32_t* real_in_fake, float* real_min_d2, int32_t* real_min_j);

}  // namespace dmvae
