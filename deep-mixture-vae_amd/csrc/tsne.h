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

// the O(N) kernels of one iteration, defined in tsne.hip and launched by tsne_knn.hip as well (the kNN-sparse form leaves the same acc / zrow)
__global__ void tsne_sum_kernel(const double* __restrict__ in, int n, double* __restrict__ out);
__global__ void tsne_grad_kernel(int N, const float4* __restrict__ acc, const double* __restrict__ Z, float e, float* __restrict__ grad);
__global__ void tsne_update_kernel(int N, const float4* __restrict__ acc, const double* __restrict__ Z, float e, float m, float lr, float* __restrict__ Y,
                                   float* __restrict__ U, float* __restrict__ G);
__global__ void tsne_init_kernel(int n2, const float* Y0, uint64_t seed, float* Y, float* __restrict__ U, float* __restrict__ G);

// ---- the kNN-sparse form (tsne_knn.hip): conditional p over the k nearest rows, the joint P as CSR, exact repulsion over all pairs ----
constexpr int TSNE_KNN_TILE = 1024;             // columns of one LDS tile of the repulsion pass: f32 sums inside it, tiles joined in order
constexpr int TSNE_KNN_MAX_SPLITS = 64;

int tsne_knn_check(const dmvae_tsne_knn_config* c, const char* who);
int tsne_knn_splits(const dmvae_tsne_knn_config* c);           // col_splits, or the choice for N when it is 0
int64_t tsne_knn_ws_bytes(const dmvae_tsne_knn_config* c);
int tsne_knn_cond_p_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const float* d2, int64_t ldd, float* p, int64_t ldp, float* beta);
int tsne_knn_gradient_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, void* ws,
                             int64_t ws_bytes, const float* Y, float exaggeration, float* grad);
int tsne_knn_step_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, void* ws,
                         int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration, float momentum);
int tsne_knn_fit_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, const float* Y0,
                        void* ws, int64_t ws_bytes, float* Y, double* kl);

}  // namespace dmvae
