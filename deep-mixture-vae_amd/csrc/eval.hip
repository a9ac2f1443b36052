// What a plan computes without a gradient (plan.h): encode, decode, the MoE prediction, and the two evaluators on the loaded batch.
#include "plan.h"
#include "eval_clusters.h"
#include "eval_loglik.h"

using namespace dmvae;

extern "C" int dmvae_plan_encode(dmvae_plan* p, void* stream, int n_valid) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_encode: plan not bound");
    (void)n_valid;
    return encode_impl(p, (hipStream_t)stream);
}

// the output layer off the last decoder activation into the f32 "recon" buffer: logits (BIAS_F32) or their sigmoid
static int output_layer_fwd(dmvae_plan* p, hipStream_t s, int kind) { return fwd_dense(p, s, p->a.dec.back(), p->out, kind, p->a.recon); }

extern "C" int dmvae_plan_decode(dmvae_plan* p, void* stream, const float* Z, int64_t ldz, int n_valid) {
    DMVAE_REQUIRE(p && p->bound && Z, "dmvae_plan_decode: plan not bound / null Z");
    DMVAE_REQUIRE(n_valid >= 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_decode: n_valid=%d exceeds max_batch", n_valid);
    hipStream_t s = (hipStream_t)stream;
    // Z (f32, caller) -> padded act buffer: a row gather with identity order
    const bool bf = p->cfg.dtype == DMVAE_BF16;
    DMVAE_REQUIRE(ldz == p->cfg.latent_dim, "dmvae_plan_decode: Z must be contiguous [n][latent_dim]");
    TRY(gather_launch(s, p->cfg.dtype, Z, n_valid, p->cfg.latent_dim, nullptr, 0, p->cfg.max_batch, n_valid, p->Bp, bf ? (void*)WS(p, p->a.Z) : nullptr, p->a.Z.ld,
                      WSf(p, bf ? p->a.Zf : p->a.Z), p->a.Z.ld, p->a.Z.ld, nullptr));
    TRY(decode_hidden(p, s));
    return output_layer_fwd(p, s, p->cfg.input_type == 0 ? DMVAE_EPI_BIAS_SIGMOID : DMVAE_EPI_BIAS_F32);
}

extern "C" int dmvae_plan_moe_predict(dmvae_plan* p, void* stream, int n_valid) {
    DMVAE_REQUIRE(p && p->bound && p->moe.on, "dmvae_plan_moe_predict: plan not bound / no MoE attachment");
    DMVAE_REQUIRE(n_valid > 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_moe_predict: n_valid=%d out of range", n_valid);
    DMVAE_REQUIRE(!p->tsrc_valid, "dmvae_plan_moe_predict: load the batch with dmvae_plan_load_batch");
    hipStream_t s = (hipStream_t)stream;
    TRY(encode_impl(p, s));
    return moe_stage(p, s, n_valid, 1.f / n_valid, false);
}

// get_accuracy on the device (eval_clusters.hip): the encoder on the loaded batch, then the confusion-matrix count on the logits (DMVAE, with or
// without a MoE attachment) or on VaDE's averaged responsibilities of `draws` samples (one encoder pass; w goes to the "eval_w" view: the logits
// buffer, which a VaDE plan allocates and never writes).  Every argument is checked before anything is enqueued.
extern "C" int dmvae_plan_eval_clusters(dmvae_plan* p, void* stream, int n_valid, const int32_t* classes, int64_t n_rows, const int32_t* perm,
                                        int64_t first, int draws, const float* eps, int64_t ld_eps, uint64_t eval_counter, int32_t* conf, int R,
                                        int32_t* err_flag) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_eval_clusters: plan not bound");
    DMVAE_REQUIRE(n_valid >= 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_eval_clusters: n_valid=%d exceeds max_batch=%d", n_valid, p->cfg.max_batch);
    hipStream_t s = (hipStream_t)stream;
    const EvalRows rows{classes, n_rows, perm, first, n_valid, conf, R, err_flag};
    if (!p->vade) {
        TRY(eval_rows_check(rows, p->cfg.n_classes, "dmvae_plan_eval_clusters"));
        TRY(encode_impl(p, s));
        return confusion_add_launch(s, WSf(p, p->a.lg), p->a.lg.ld, p->cfg.n_classes, rows);
    }
    VadeEvalArgs a;
    latent_inputs(p, a, eps, ld_eps);
    a.rows = rows;
    a.draws = draws; a.counter = eval_counter;
    a.w = WSf(p, p->a.lg); a.ld_w = p->a.lg.ld;
    a.ws = p->lws_bytes ? WSf(p, p->o_lws) : nullptr; a.ws_bytes = p->lws_bytes;
    TRY(vade_eval_check(a, "dmvae_plan_eval_clusters"));
    TRY(encode_impl(p, s));
    return vade_eval_launch(s, a);
}

// Held-out log-likelihood of the loaded batch (eval_loglik.hip): the importance-weighted bound with `draws` samples per row.  One encoder pass, then per
// draw {z_s and log p(z_s) - log q_s, the decoder's hidden layers, the output layer's f32 logits into the "recon" buffer, the row sums and the running
// logsumexp}, then the rows' L and their sum.  Reads parameters; writes activation views and the caller's scratch only: no gradient, no state change.
extern "C" int64_t dmvae_plan_eval_loglik_ws_bytes(const dmvae_plan* p) { return p ? loglik_ws_bytes(p->Bp) : (int64_t)DMVAE_EINVAL; }

extern "C" int dmvae_plan_eval_loglik(dmvae_plan* p, void* stream, int n_valid, int64_t n_rows, int64_t first, int draws, const float* eps, int64_t ld_eps,
                                      uint64_t eval_counter, void* ws, int64_t ws_bytes, float* row_ll, double* acc) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_eval_loglik: plan not bound");
    DMVAE_REQUIRE(n_valid >= 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_eval_loglik: n_valid=%d exceeds max_batch=%d", n_valid, p->cfg.max_batch);
    DMVAE_REQUIRE(draws >= 1 && draws <= LOGLIK_MAX_DRAWS, "dmvae_plan_eval_loglik: draws=%d (1 .. %d)", draws, LOGLIK_MAX_DRAWS);
    DMVAE_REQUIRE(first >= 0 && first + n_valid <= n_rows, "dmvae_plan_eval_loglik: rows [%lld, %lld + %d) are not inside the %lld rows of the data set",
                  (long long)first, (long long)first, n_valid, (long long)n_rows);
    DMVAE_REQUIRE(!eps || ld_eps >= p->cfg.latent_dim, "dmvae_plan_eval_loglik: ld_eps=%lld < latent_dim=%d", (long long)ld_eps, p->cfg.latent_dim);
    const int64_t need = loglik_ws_bytes(p->Bp);
    DMVAE_REQUIRE(ws && ws_bytes >= need && (uintptr_t)ws % 4 == 0, "dmvae_plan_eval_loglik: the scratch holds %lld bytes, %lld are needed (dmvae_plan_eval_loglik_ws_bytes)",
                  (long long)(ws ? ws_bytes : 0), (long long)need);
    DMVAE_REQUIRE(acc, "dmvae_plan_eval_loglik: null acc");
    DMVAE_REQUIRE(!p->tsrc_valid, "dmvae_plan_eval_loglik: load the batch with dmvae_plan_load_batch (the f32 copy of the batch holds the targets)");
    hipStream_t s = (hipStream_t)stream;
    const dmvae_config& c = p->cfg;
    float* a_s = reinterpret_cast<float*>(ws);
    float* run_m = a_s + p->Bp;
    float* run_s = run_m + p->Bp;
    LoglikDrawArgs a;
    memset(&a, 0, sizeof(a));
    latent_inputs(p, a, eps, ld_eps);
    latent_sample(p, a);
    a.n_valid = n_valid; a.act_dtype = c.dtype;
    a.n_rows = n_rows; a.first = first;
    a.counter = eval_counter;
    a.a_out = a_s;
    if (n_valid == 0) return 0;
    TRY(encode_impl(p, s));
    for (int d = 0; d < draws; ++d) {
        a.draw = d;
        TRY(loglik_draw_launch(s, a));
        TRY(decode_hidden(p, s));
        TRY(output_layer_fwd(p, s, DMVAE_EPI_BIAS_F32));
        TRY(loglik_rows_launch(s, WSf(p, p->a.recon), WSf(p, p->a.xf), p->a.recon.ld, c.input_dim, n_valid, c.input_type, d, a_s, run_m, run_s));
    }
    return loglik_finish_launch(s, run_m, run_s, n_valid, draws, row_ll, acc);
}
