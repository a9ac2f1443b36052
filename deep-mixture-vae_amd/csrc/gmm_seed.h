// k-means++ seeding of the mixture fit on the device (gmm_seed.hip): host-side launchers, namespace dmvae.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int GMM_SEED_MAX_BLOCKS = 256;      // row workgroups per restart: their f64 partials are scanned by ONE 256-thread workgroup
constexpr int GMM_SEED_MAX_TRIALS = 8;        // candidates per centre (sklearn's 2 + int(ln K) is <= 8 up to K = 1096)
constexpr int GMM_SEED_PHILOX_STREAM = 3;     // 0, 1: the steps' eps / Gumbel noise; 2: the evaluation's draws
constexpr int GMM_SEED_LDS_FIXED = 4096;      // reduction scratch next to the staged candidate rows

// 0 when the shape fits, else DMVAE_EINVAL / DMVAE_EUNSUPPORTED with the error text set
int gmm_seed_check(const dmvae_gmm_seed_config* c, const char* who);
int gmm_seed_trials(const dmvae_gmm_seed_config* c);      // T: local_trials, or 2 + int(ln K) when it is 0
int64_t gmm_seed_ws_bytes(const dmvae_gmm_seed_config* c);
int gmm_seed_launch(hipStream_t s, const dmvae_gmm_seed_config* c, const float* X, int64_t ldx, const float* u, void* ws, int64_t ws_bytes,
                    float* centers, int32_t* rows);

}  // namespace dmvae
