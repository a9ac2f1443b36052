// Cluster quality on the device (cluster_metrics.hip): per-row labels and the silhouette coefficient; host-side launchers, namespace dmvae.
#pragma once
#include "common.h"
#include "eval_clusters.h"

namespace dmvae {

constexpr int SIL_MAX_N = 1 << 20;
constexpr int SIL_MAX_K = EVAL_MAX_R;            // the labels are arg-maxes of at most EVAL_MAX_R scores
constexpr int SIL_ERR_LABEL = 1;                 // err_flag bit: a label outside [0, K)

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int argmax_labels_launch(hipStream_t s, const float* scores, int64_t ld, int n_valid, int K, int32_t* labels);
int64_t silhouette_ws_bytes(int64_t n, int K);   // < 0: DMVAE_EINVAL
int silhouette_launch(hipStream_t s, const float* Z, int64_t ldz, int n, int D, const int32_t* labels, int K, void* ws, int64_t ws_bytes,
                      float* samples, double* out, int32_t* err_flag);

}  // namespace dmvae
