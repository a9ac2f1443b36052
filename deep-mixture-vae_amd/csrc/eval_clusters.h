// Clustering evaluation on the device (eval_clusters.hip): host-side launchers, namespace dmvae.
#pragma once
#include "common.h"

namespace dmvae {

constexpr uint32_t EVAL_PHILOX_STREAM = 2u;      // the steps draw their normals from stream 0 and their Gumbel noise from stream 1
constexpr int EVAL_MAX_R = 4096;                 // side of the confusion matrix (R * R int32 counts)
constexpr int EVAL_MAX_DRAWS = 1024;

// err_flag bits
constexpr int EVAL_ERR_CLASS = 1;                // a class outside [0, R)
constexpr int EVAL_ERR_PERM = 2;                 // a permutation entry outside [0, n_rows)

// where the class of batch row r comes from: classes[perm ? perm[first + r] : first + r], as the gather of the batch reads its rows
struct EvalRows {
    const int32_t* classes; int64_t n_rows; const int32_t* perm; int64_t first; int n_valid;
    int32_t* conf; int R; int32_t* err_flag;
};

struct VadeEvalArgs {
    EvalRows rows;
    int D, K, draws;
    const float* mean; int64_t ld_mean;
    const float* log_var; int64_t ld_log_var;
    const float* prior_means; const float* prior_log_vars;      // [K][D]
    const float* eps; int64_t ld_eps;                           // [draws][n_valid][ld_eps] or nullptr: Philox
    uint64_t seed, counter;
    float* w; int64_t ld_w;                                     // [n_valid][>= K] averaged responsibilities
    // tables past the LDS limit of vade_eval_kernel (latent_vade_mfma_needed): the scratch of the large-table form for B_pad rows
    // (latent_vade_mfma_ws_bytes), B_pad % 64 == 0 and >= n_valid; not read otherwise
    int B_pad; float* ws; int64_t ws_bytes;
};

// 0, or DMVAE_EINVAL / DMVAE_EUNSUPPORTED with the error text set (nothing is enqueued)
int eval_rows_check(const EvalRows& r, int K, const char* who);
int vade_eval_check(const VadeEvalArgs& a, const char* who);
int confusion_add_launch(hipStream_t s, const float* scores, int64_t ld, int K, const EvalRows& r);
int vade_eval_launch(hipStream_t s, const VadeEvalArgs& a);
int vade_eval_mfma_launch(hipStream_t s, const VadeEvalArgs& a);      // latent_vade_mfma.hip; through vade_eval_launch only

}  // namespace dmvae
