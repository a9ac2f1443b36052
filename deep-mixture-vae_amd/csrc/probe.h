// Linear probe of the latent means on the device (probe.hip): host-side launchers of the softmax-regression evaluation and of its scores.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int64_t PROBE_MAX_N = (int64_t)1 << 22;
constexpr int PROBE_MAX_D = 512;
constexpr int PROBE_MAX_C = 256;
constexpr int PROBE_MAX_DC = 16384;              // W is at most 64 KiB (70 KiB with b and the pad columns): it sits in LDS beside a row tile
constexpr int PROBE_ERR = 1;                     // flag bit: a class outside [0, C)

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int64_t probe_xent_ws_bytes(int64_t n, int D, int C);          // < 0: DMVAE_EINVAL
int probe_xent_launch(hipStream_t s, const float* Z, int64_t ldz, int64_t n, int D, const float* shift, const float* scale, const int32_t* classes, int C,
                      const float* W, int64_t ldw, const float* b, void* ws, int64_t ws_bytes, double* out, int32_t* flag);
int probe_scores_launch(hipStream_t s, const float* Z, int64_t ldz, int M, int D, const float* shift, const float* scale, const float* W, int64_t ldw,
                        const float* b, int C, float* scores, int64_t lds);

}  // namespace dmvae
