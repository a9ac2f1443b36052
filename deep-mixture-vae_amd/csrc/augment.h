// Random affine warp of the resident rows on the device (augment.hip): every row a single-plane H x W image, warped by its own map.  Host-side launcher.
#pragma once
#include "common.h"

namespace dmvae {

constexpr uint32_t AUGMENT_PHILOX_STREAM = 9u;   // 0 .. 8 are taken: the table of DESIGN.md section 4
constexpr int AUGMENT_MAX_SIDE = 64;             // H, W <= 64: an image is at most 16 KiB of LDS
constexpr int64_t AUGMENT_MAX_BLOCK = (int64_t)1 << 56;      // two blocks per data-set row, below the stream bits

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int augment_rows_launch(hipStream_t s, const float* X, int64_t ldx, int64_t n_rows, int H, int W, int64_t row_base, uint64_t seed, uint64_t counter,
                        const dmvae_augment_params* p, const float* theta_in, float* theta_out, float* out, int64_t ldo);

}  // namespace dmvae
