// Diagonal-covariance Gaussian mixture fit on the device (gmm_fit.hip): host-side launchers, namespace dmvae.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int GMM_TILE_ROWS = 32;       // rows staged in LDS per trip of a row-stage workgroup
constexpr int GMM_MAX_BLOCKS = 256;     // row-stage workgroups per restart (a function of N alone: restarts run side by side bit for bit)
constexpr int GMM_PAIRS_PER_THREAD = 13;   // (k, d) statistics a thread keeps in registers: K * D <= 256 * 13

// 0 when the shape fits, else DMVAE_EINVAL / DMVAE_EUNSUPPORTED with the error text set
int gmm_check(const dmvae_gmm_config* c, const char* who);
int64_t gmm_ws_bytes(const dmvae_gmm_config* c);
int gmm_fit_launch(hipStream_t s, const dmvae_gmm_config* c, const float* X, int64_t ldx, const int32_t* labels, const float* centers,
                   const float* weights_init, void* ws, int64_t ws_bytes, const dmvae_gmm_result* out, bool kmeans_only);

}  // namespace dmvae
