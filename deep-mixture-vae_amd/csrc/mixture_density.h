// Log-density of points under a diagonal Gaussian mixture with any number of components, posterior samples and the column statistics
// of the encoder outputs (mixture_density.hip): host-side launchers, namespace dmvae.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int MD_MAX_ROWS = 1 << 20;             // points, components and rows per call
constexpr uint32_t MD_PHILOX_STREAM = 6;         // posterior_sample's noise stream

// the J split of mixture_logpdf: a function of (M, J, D) alone
struct MdSplit { int tiles, tiles_per_split, nsplit; };
MdSplit mixture_logpdf_split(int M, int J, int D);

// 0 (a size: >= 0), or DMVAE_EINVAL with the error text set (nothing is enqueued)
int64_t mixture_logpdf_ws_bytes(int64_t M, int64_t J, int64_t D);
int mixture_logpdf_launch(hipStream_t s, const float* Z, int64_t ldz, int M, int D, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int J,
                          const float* log_w, void* ws, int64_t ws_bytes, float* out);
int posterior_sample_launch(hipStream_t s, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, const float* eps, int64_t ld_eps,
                            uint64_t seed, uint64_t counter, int64_t pos0, float* Z, int64_t ldz, float* logq);
int64_t column_stats_ws_bytes(int64_t n, int64_t D);
int column_stats_launch(hipStream_t s, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, void* ws, int64_t ws_bytes, double* out);
int sum_f64_launch(hipStream_t s, const float* x, int64_t n, double* out);

}  // namespace dmvae
