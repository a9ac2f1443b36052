// Held-out log-likelihood on the device (eval_loglik.hip): host-side launchers, namespace dmvae.
#pragma once
#include "common.h"

namespace dmvae {

constexpr uint32_t LOGLIK_PHILOX_STREAM = 4u;    // 0 / 1: the steps' normals and Gumbel noise, 2: eval_clusters.hip, 3: gmm_seed.hip
constexpr int LOGLIK_MAX_DRAWS = 1024;

// one draw s of the importance-weighted bound for the rows of a batch: z_s and a_s = log p(z_s) - log q(z_s | x)
struct LoglikDrawArgs {
    int n_valid, B_pad, D, K, act_dtype, draw;
    int64_t n_rows, first;                                      // the row's position in the evaluated order: first + r of n_rows
    const float* mean; int64_t ld_mean;
    const float* log_var; int64_t ld_log_var;
    const float* prior_means; const float* prior_log_vars;      // [K][D]
    const float* eps; int64_t ld_eps;                           // [draws][n_valid][ld_eps] or nullptr: Philox
    uint64_t seed, counter;
    void* Z_act; int64_t ld_Z;                                  // [B_pad][ld_Z] act dtype: pad columns and rows >= n_valid are zeroed
    float* Z_f32; int64_t ld_Zf;                                // bf16 plans: the f32 z (nullptr: Z_act is f32)
    float* a_out;                                               // [B_pad], rows < n_valid
};

// the caller's scratch for B_pad rows: a_s | running max | running scaled sum, one float each per row
int64_t loglik_ws_bytes(int B_pad);
// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int loglik_draw_launch(hipStream_t s, const LoglikDrawArgs& a);
// w_s = log p(x | z_s) + a_s of rows < n_valid from the f32 logits / targets [..][ld], columns < I; the rows' running logsumexp over the draws
int loglik_rows_launch(hipStream_t s, const float* logits, const float* x, int64_t ld, int I, int n_valid, int recon_kind, int draw,
                       const float* a_s, float* run_m, float* run_s);
// L_r = m + log(sum) - log(draws) -> row_ll (or nullptr); acc[0] += sum_r L_r, acc[1] += n_valid (double, fixed-order tree)
int loglik_finish_launch(hipStream_t s, const float* run_m, const float* run_s, int n_valid, int draws, float* row_ll, double* acc);

}  // namespace dmvae
