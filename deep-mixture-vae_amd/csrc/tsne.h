// Exact t-SNE on the device (tsne.hip): host-side launchers, namespace dmvae.
#pragma once
#include "common.h"

namespace dmvae {

constexpr uint32_t TSNE_PHILOX_STREAM = 5u;     // 0 / 1: the steps' normals and Gumbel noise, 2: eval_clusters.hip, 3: gmm_seed.hip, 4: eval_loglik.hip
constexpr int TSNE_MAX_N = 32768;               // N * N floats = 4 GiB; every index into them is 64-bit
constexpr int TSNE_SEARCH_STEPS = 64;           // bisection steps of the perplexity search: always all of them

// 0 when the shape is accepted, else DMVAE_EINVAL / DMVAE_EUNSUPPORTED with the error text set
int tsne_check(const dmvae_tsne_config* c, const char* who);
int64_t tsne_ws_bytes(const dmvae_tsne_config* c);
int tsne_joint_p_launch(hipStream_t s, const dmvae_tsne_config* c, const float* X, int64_t ldx, void* ws, int64_t ws_bytes, float* beta);
int tsne_gradient_launch(hipStream_t s, const dmvae_tsne_config* c, void* ws, int64_t ws_bytes, const float* Y, float exaggeration, float* grad);
int tsne_step_launch(hipStream_t s, const dmvae_tsne_config* c, void* ws, int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration,
                     float momentum);
int tsne_fit_launch(hipStream_t s, const dmvae_tsne_config* c, const float* X, int64_t ldx, const float* Y0, void* ws, int64_t ws_bytes, float* Y,
                    double* kl);

}  // namespace dmvae
