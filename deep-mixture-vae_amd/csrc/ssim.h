// Structural similarity on the device (ssim.hip): the per-row SSIM and squared error of two sets of image rows.  Host-side launcher.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int SSIM_ERR_INDEX = 2;                // err_flag bit 1: an ix / iy entry outside its row set (bit 1 as the evaluators' perm entries)
constexpr int SSIM_MAX_WIN = 11;                 // odd windows 3 .. 11
constexpr int SSIM_MAX_HW = 4096;                // the two planes of a pair in LDS: 2 * 4096 * 4 B = 32 KiB

// 0, or DMVAE_EINVAL / DMVAE_EUNSUPPORTED with the error text set (nothing is enqueued)
int ssim_rows_launch(hipStream_t s, const float* X, int64_t ldx, int64_t nx, const int32_t* ix, const float* Y, int64_t ldy, int64_t ny, const int32_t* iy,
                     int64_t n_pairs, int H, int W, int planes, const float* w1, int win, float c1, float c2, float* ssim, float* sse, int32_t* err_flag);

}  // namespace dmvae
