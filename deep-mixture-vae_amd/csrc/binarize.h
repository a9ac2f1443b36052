// Binarisation of the resident rows on the device (binarize.hip): the Bernoulli draw and the fixed threshold.  Host-side launcher.
#pragma once
#include "common.h"

namespace dmvae {

constexpr uint32_t BINARIZE_PHILOX_STREAM = 8u;  // 0 .. 7 are taken: the table of DESIGN.md section 4
constexpr int64_t BINARIZE_MAX_FLAT = (int64_t)1 << 58;      // flat indices below this: block indices below 2^56, clear of the stream bits
enum { BINARIZE_BERNOULLI = 0, BINARIZE_THRESHOLD = 1 };

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int binarize_rows_launch(hipStream_t s, const float* X, int64_t ldx, int64_t n_rows, int n_cols, int64_t row_base, uint64_t seed, uint64_t counter,
                         int mode, float* out, int64_t ldo);

}  // namespace dmvae
