// extern "C" surface of libdmvae_hip.so (include/dmvae_hip.h) outside the step plan: errors, HIP-event profiling of every
// launch, the checked GEMM entry, the thin wrappers over the launchers and the debug knobs.  The plan lives in plan.hip (layout),
// step.hip (the training pass) and eval.hip (encode / decode / evaluators).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "plan.h"
#include "gmm_fit.h"
#include "gmm_seed.h"
#include "eval_clusters.h"
#include "eval_loglik.h"
#include "tsne.h"
#include "cluster_metrics.h"
#include "mixture_density.h"
#include "knn.h"
#include "prdc.h"
#include "sinkhorn.h"
#include "binarize.h"
#include "augment.h"
#include "ssim.h"
#include "probe.h"
#include "label_xent.h"
#include "label_spread.h"
#include "measure.h"

namespace dmvae {

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// ------------------------------------------------------------------ profiling
// One record per ProfScope: the event BRACKET around the scope's launches (e0, e1: holds the launches' dispatch besides the
// kernels) and, per kernel launched inside it, the pair bound to that dispatch (k: the kernel's own begin -> end).
struct ProfRec { const char* name; double flops, bytes; hipEvent_t e0, e1; std::vector<std::pair<hipEvent_t, hipEvent_t>> k; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_event_pool;
static std::mutex g_prof_mu;
static thread_local int g_prof_cur = -1;       // slot of the innermost open ProfScope of this thread

static hipEvent_t get_event() {
    if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
ProfScope::ProfScope(hipStream_t s_, const char* name, double flops, double bytes) : s(s_), slot(-1), outer(-1) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec r{name, flops, bytes, get_event(), get_event(), {}};
    (void)hipEventRecord(r.e0, s);
    slot = (int)g_prof.size();
    g_prof.push_back(r);
    outer = g_prof_cur;
    g_prof_cur = slot;
}
ProfScope::~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    (void)hipEventRecord(g_prof[slot].e1, s);
    g_prof_cur = outer;
}
bool prof_launch_events(hipEvent_t* e0, hipEvent_t* e1) {
    if (!g_prof_on || g_prof_cur < 0) return false;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_cur >= (int)g_prof.size()) return false;
    *e0 = get_event();
    *e1 = get_event();
    g_prof[g_prof_cur].k.emplace_back(*e0, *e1);
    return true;
}

static const char* gemm_name(int dtype, int layout) {
    static const char* n[2][3] = {{"gemm_f32_fwd", "gemm_f32_dx", "gemm_f32_dw"}, {"gemm_bf16_fwd", "gemm_bf16_dx", "gemm_bf16_dw"}};
    return n[dtype][layout];
}

int gemm_checked(hipStream_t s, int dtype, int layout, int M, int N, int K, const void* A, int64_t lda,
                 const void* B, int64_t ldb, const dmvae_epilogue* epi, int split, GemmArgs* deferred, int conv_p, int conv_c) {
    DMVAE_REQUIRE(dtype == DMVAE_F32 || dtype == DMVAE_BF16, "dmvae_gemm: bad dtype %d", dtype);
    DMVAE_REQUIRE(layout >= 0 && layout <= 2, "dmvae_gemm: bad layout %d", layout);
    DMVAE_REQUIRE(A && B && epi && epi->out, "dmvae_gemm: null pointer");
    DMVAE_REQUIRE(M > 0 && N > 0 && K > 0 && M % 64 == 0 && N % 64 == 0 && K % 64 == 0,
                  "dmvae_gemm: M=%d N=%d K=%d must be positive multiples of 64 (pad the operands)", M, N, K);
    DMVAE_REQUIRE(split >= 1 && K % (split * 64) == 0, "dmvae_gemm: split_k=%d does not divide K=%d into multiples of 64", split, K);
    DMVAE_REQUIRE(split == 1 || epi->kind == DMVAE_EPI_ATOMIC_F32, "dmvae_gemm: split_k > 1 needs DMVAE_EPI_ATOMIC_F32");
    const int esz = dtype == DMVAE_BF16 ? 2 : 4;
    DMVAE_REQUIRE(((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0) && (lda * esz) % 16 == 0 && (ldb * esz) % 16 == 0,
                  "dmvae_gemm: operands must be 16-byte aligned with 16-byte multiple row strides");
    GemmArgs a;
    a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    a.M = M; a.N = N; a.K = K; a.k_split = K / split; a.group_m = 8;
    a.conv_p = conv_p; a.conv_c = conv_c;
    DMVAE_REQUIRE(conv_c == 0 || ((conv_c == 32 || conv_c % 64 == 0) && lda >= conv_c &&
                                  (layout == DMVAE_GEMM_DW ? M == pad64(9 * conv_c) : (K == pad64(9 * conv_c) && split == 1))),
                  "dmvae_gemm: conv mode: 32 or a multiple of 64 channels per tap (<= lda), 9 taps padded to 64 along K (M for the weight gradient)");
    a.epi = *epi;
    if (a.epi.m_valid <= 0) a.epi.m_valid = M;
    if (a.epi.n_valid <= 0) a.epi.n_valid = N;
    if (deferred) { *deferred = a; return 0; }      // caller batches it into a grouped launch
    if (dtype == DMVAE_BF16) return gemm_bf16_dispatch(s, layout, a, split);   // (profiled per template instantiation inside)
    const double bytes = 4.0 * ((double)M * K + (double)K * N + (double)M * N);
    ProfScope ps(s, gemm_name(dtype, layout), 2.0 * M * N * (double)K, bytes);
    return gemm_f32_dispatch(s, layout, a, split);
}

int gemm_partials(int, int M, int N) { return (M / 64) * (N / 64); }

}  // namespace dmvae

using namespace dmvae;

// ====================================================================== thin C wrappers
extern "C" int dmvae_gemm(void* stream, int dtype, int layout, int M, int N, int K, const void* A, int64_t lda,
                          const void* B, int64_t ldb, const dmvae_epilogue* epi, int split_k) {
    DMVAE_REQUIRE(!epi || (epi->recon_kind == 0 || epi->recon_kind == 1), "dmvae_gemm: recon_kind %d (0 binary, 1 real)", epi ? epi->recon_kind : 0);
    return gemm_checked((hipStream_t)stream, dtype, layout, M, N, K, A, lda, B, ldb, epi, split_k);
}
extern "C" int dmvae_gemm_partials(int dtype, int M, int N) { return gemm_partials(dtype, M, N); }

extern "C" int dmvae_gemm_grouped(void* stream, int dtype, int layout, const dmvae_gemm_problem* probs, int n) {
    DMVAE_REQUIRE(probs && n >= 1 && n <= DMVAE_MAX_GROUP, "dmvae_gemm_grouped: 1..%d problems", DMVAE_MAX_GROUP);
    hipStream_t s = (hipStream_t)stream;
    std::vector<GemmArgs> q(n);
    for (int i = 0; i < n; ++i) {
        const dmvae_gemm_problem& pr = probs[i];
        if (dtype == DMVAE_BF16) TRY(gemm_checked(s, dtype, layout, pr.M, pr.N, pr.K, pr.A, pr.lda, pr.B, pr.ldb, &pr.epi, 1, &q[i]));
        else TRY(gemm_checked(s, dtype, layout, pr.M, pr.N, pr.K, pr.A, pr.lda, pr.B, pr.ldb, &pr.epi, 1));   // f32: one launch each
    }
    return dtype == DMVAE_BF16 ? gemm_bf16_grouped(s, layout, q.data(), n) : 0;
}
extern "C" int dmvae_gemm_grouped_dw(void* stream, int dtype, const dmvae_gemm_problem* probs, int n) {
    DMVAE_REQUIRE(probs && n >= 1, "dmvae_gemm_grouped_dw: no problems");
    for (int i = 0; i < n; ++i)
        DMVAE_REQUIRE(probs[i].epi.kind == DMVAE_EPI_STORE_F32, "dmvae_gemm_grouped_dw: problems must use DMVAE_EPI_STORE_F32");
    return dmvae_gemm_grouped(stream, dtype, DMVAE_GEMM_DW, probs, n);
}
extern "C" int dmvae_gemm_grouped_dw_adam(void* stream, const dmvae_gemm_problem* probs, int n, const dmvae_adam_ctx* ctx) {
    DMVAE_REQUIRE(probs && ctx && n >= 1 && n <= DMVAE_MAX_GROUP, "dmvae_gemm_grouped_dw_adam: 1..%d problems and a context", DMVAE_MAX_GROUP);
    hipStream_t s = (hipStream_t)stream;
    std::vector<GemmArgs> q(n);
    for (int i = 0; i < n; ++i) {
        const dmvae_gemm_problem& pr = probs[i];
        TRY(gemm_checked(s, DMVAE_BF16, DMVAE_GEMM_DW, pr.M, pr.N, pr.K, pr.A, pr.lda, pr.B, pr.ldb, &pr.epi, 1, &q[i]));
    }
    return gemm_bf16_grouped_dw_adam(s, q.data(), n, *ctx);
}

extern "C" int dmvae_latent_nblocks(int B_pad, int D, int K) { return latent_nblocks(B_pad, D, K); }
extern "C" int dmvae_latent_nblocks_vade(int B_pad) { return latent_vade_nblocks(B_pad); }
extern "C" int64_t dmvae_latent_ws_bytes(int B_pad, int D, int K, int mode) {
    if (mode == 2) return dmvae_latent_vade_ws_bytes(B_pad, D, K, 0, nullptr);
    return (B_pad > 0 && B_pad % 64 == 0 && latent_mfma_applies(D, K, mode)) ? latent_mfma_ws_bytes(B_pad, D, K) : 0;
}
extern "C" int64_t dmvae_latent_vade_ws_bytes(int B_pad, int D, int K, int forced, int* n_slabs) {
    if (n_slabs) *n_slabs = 0;
    if (B_pad <= 0 || B_pad % 64 != 0 || D < 1 || K < 1 || (!forced && !latent_vade_mfma_needed(D, K))) return 0;
    return latent_vade_mfma_ws_bytes(B_pad, D, K, n_slabs);
}
extern "C" int dmvae_latent_fwd(void* stream, const dmvae_latent_args* a) {
    DMVAE_REQUIRE(a && a->mode >= 0 && a->mode <= 2, "dmvae_latent_fwd: bad mode %d", a ? a->mode : -1);
    DMVAE_REQUIRE(a->mean && a->log_var && (a->logits || a->mode == 2) && a->prior_means && a->prior_log_vars && a->Z_act && a->gmu && a->glv &&
                  a->clv && (a->dlogits_act || a->mode == 2) && a->dprior_partials && a->loss_partials, "dmvae_latent_fwd: null pointer");
    DMVAE_REQUIRE(a->ld_Z >= a->D && (a->ld_dl >= a->K || a->mode == 2) && a->ld_g >= a->D, "dmvae_latent_fwd: leading dimension too small");
    return latent_launch((hipStream_t)stream, a);
}
extern "C" int64_t dmvae_heads_latent_kslice_floats(int B_pad, int Dp, int kslices) { return heads_latent_kslice_floats(B_pad, Dp, kslices); }
extern "C" int dmvae_heads_latent_ok(int B_pad, int D, int K, int Dp, int Kp, int Hp, int mode) { return heads_latent_ok(B_pad, D, K, Dp, Kp, Hp, mode, 16) ? 1 : 0; }
extern "C" int dmvae_heads_latent_fwd(void* stream, const dmvae_heads_args* h, const dmvae_latent_args* a) {
    DMVAE_REQUIRE(h && a && a->mode >= 0 && a->mode <= 1, "dmvae_heads_latent_fwd: bad arguments / mode");
    DMVAE_REQUIRE(h->hz && h->W_mv && h->W_lg && h->b_mv && h->b_lg && a->mean && a->log_var && a->logits && a->prior_means && a->prior_log_vars && a->Z_act && a->gmu &&
                  a->glv && a->clv && a->dlogits_act && a->dprior_partials && a->loss_partials, "dmvae_heads_latent_fwd: null pointer");
    DMVAE_REQUIRE(a->ld_Z >= a->D && a->ld_dl >= a->K && a->ld_g >= a->D, "dmvae_heads_latent_fwd: leading dimension too small");
    return heads_latent_launch((hipStream_t)stream, a, h);
}
extern "C" int64_t dmvae_gmm_ws_bytes(const dmvae_gmm_config* cfg) {
    if (int rc = gmm_check(cfg, "dmvae_gmm_ws_bytes")) return rc;
    return gmm_ws_bytes(cfg);
}
extern "C" int dmvae_gmm_fit(void* stream, const dmvae_gmm_config* cfg, const float* X, int64_t ldx, const int32_t* labels, const float* centers,
                             const float* weights_init, void* ws, int64_t ws_bytes, dmvae_gmm_result* out) {
    return gmm_fit_launch((hipStream_t)stream, cfg, X, ldx, labels, centers, weights_init, ws, ws_bytes, out, false);
}
extern "C" int dmvae_gmm_kmeans(void* stream, const dmvae_gmm_config* cfg, const float* X, int64_t ldx, const float* centers, void* ws,
                                int64_t ws_bytes, dmvae_gmm_result* out) {
    return gmm_fit_launch((hipStream_t)stream, cfg, X, ldx, nullptr, centers, nullptr, ws, ws_bytes, out, true);
}
extern "C" int64_t dmvae_gmm_seed_ws_bytes(const dmvae_gmm_seed_config* cfg) {
    if (int rc = gmm_seed_check(cfg, "dmvae_gmm_seed_ws_bytes")) return rc;
    return gmm_seed_ws_bytes(cfg);
}
extern "C" int dmvae_gmm_seed(void* stream, const dmvae_gmm_seed_config* cfg, const float* X, int64_t ldx, const float* u, void* ws, int64_t ws_bytes,
                              float* centers, int32_t* rows) {
    return gmm_seed_launch((hipStream_t)stream, cfg, X, ldx, u, ws, ws_bytes, centers, rows);
}
extern "C" int64_t dmvae_tsne_ws_bytes(const dmvae_tsne_config* cfg) {
    if (int rc = tsne_check(cfg, "dmvae_tsne_ws_bytes")) return rc;
    return tsne_ws_bytes(cfg);
}
extern "C" int dmvae_tsne_joint_p(void* stream, const dmvae_tsne_config* cfg, const float* X, int64_t ldx, void* ws, int64_t ws_bytes, float* beta) {
    return tsne_joint_p_launch((hipStream_t)stream, cfg, X, ldx, ws, ws_bytes, beta);
}
extern "C" int dmvae_tsne_gradient(void* stream, const dmvae_tsne_config* cfg, void* ws, int64_t ws_bytes, const float* Y, float exaggeration,
                                   float* grad) {
    return tsne_gradient_launch((hipStream_t)stream, cfg, ws, ws_bytes, Y, exaggeration, grad);
}
extern "C" int dmvae_tsne_step(void* stream, const dmvae_tsne_config* cfg, void* ws, int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration,
                               float momentum) {
    return tsne_step_launch((hipStream_t)stream, cfg, ws, ws_bytes, Y, U, G, exaggeration, momentum);
}
extern "C" int dmvae_tsne_fit(void* stream, const dmvae_tsne_config* cfg, const float* X, int64_t ldx, const float* Y0, void* ws, int64_t ws_bytes,
                              float* Y, double* kl) {
    return tsne_fit_launch((hipStream_t)stream, cfg, X, ldx, Y0, ws, ws_bytes, Y, kl);
}
extern "C" const float* dmvae_tsne_p(const void* ws) { return (const float*)ws; }
extern "C" int64_t dmvae_tsne_knn_ws_bytes(const dmvae_tsne_knn_config* cfg) {
    if (int rc = tsne_knn_check(cfg, "dmvae_tsne_knn_ws_bytes")) return rc;
    return tsne_knn_ws_bytes(cfg);
}
extern "C" int dmvae_tsne_knn_cond_p(void* stream, const dmvae_tsne_knn_config* cfg, const float* d2, int64_t ldd, float* p, int64_t ldp, float* beta) {
    return tsne_knn_cond_p_launch((hipStream_t)stream, cfg, d2, ldd, p, ldp, beta);
}
extern "C" int dmvae_tsne_knn_gradient(void* stream, const dmvae_tsne_knn_config* cfg, const int64_t* indptr, const int32_t* indices, const float* values,
                                       void* ws, int64_t ws_bytes, const float* Y, float exaggeration, float* grad) {
    return tsne_knn_gradient_launch((hipStream_t)stream, cfg, indptr, indices, values, ws, ws_bytes, Y, exaggeration, grad);
}
extern "C" int dmvae_tsne_knn_step(void* stream, const dmvae_tsne_knn_config* cfg, const int64_t* indptr, const int32_t* indices, const float* values,
                                   void* ws, int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration, float momentum) {
    return tsne_knn_step_launch((hipStream_t)stream, cfg, indptr, indices, values, ws, ws_bytes, Y, U, G, exaggeration, momentum);
}
extern "C" int dmvae_tsne_knn_fit(void* stream, const dmvae_tsne_knn_config* cfg, const int64_t* indptr, const int32_t* indices, const float* values,
                                  const float* Y0, void* ws, int64_t ws_bytes, float* Y, double* kl) {
    return tsne_knn_fit_launch((hipStream_t)stream, cfg, indptr, indices, values, Y0, ws, ws_bytes, Y, kl);
}
extern "C" int dmvae_confusion_add(void* stream, const float* scores, int64_t ld, int n_valid, int K, const int32_t* classes, int64_t n_rows,
                                   const int32_t* perm, int64_t first, int32_t* conf, int R, int32_t* err_flag) {
    return confusion_add_launch((hipStream_t)stream, scores, ld, K, EvalRows{classes, n_rows, perm, first, n_valid, conf, R, err_flag});
}
extern "C" int64_t dmvae_label_xent_acc_elems(int n_valid) { return label_xent_acc_elems(n_valid); }
extern "C" int dmvae_label_xent(void* stream, const float* logits, int64_t ld_lg, int n_valid, int K, const int32_t* labels, int64_t label_rows,
                                const int32_t* perm, int64_t first, float scale, int act_dtype, void* dlogits, int64_t ld_dl, float* row_loss,
                                double* acc, int32_t* err_flag) {
    LabelXentArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = logits; a.ld_lg = ld_lg; a.n_valid = n_valid; a.K = K;
    a.labels = labels; a.label_rows = label_rows; a.perm = perm; a.first = first;
    a.act_dtype = act_dtype; a.scale = scale;
    a.dlogits = dlogits; a.ld_dl = ld_dl; a.row_loss = row_loss; a.acc = acc; a.err_flag = err_flag;
    return label_xent_launch((hipStream_t)stream, a, "dmvae_label_xent");
}
extern "C" int dmvae_argmax_labels(void* stream, const float* scores, int64_t ld, int n_valid, int K, int32_t* labels) {
    return argmax_labels_launch((hipStream_t)stream, scores, ld, n_valid, K, labels);
}
extern "C" int64_t dmvae_silhouette_ws_bytes(int64_t n, int K) { return silhouette_ws_bytes(n, K); }
extern "C" int dmvae_silhouette(void* stream, const float* Z, int64_t ldz, int n, int D, const int32_t* labels, int K, void* ws, int64_t ws_bytes,
                                float* samples, double* out, int32_t* err_flag) {
    return silhouette_launch((hipStream_t)stream, Z, ldz, n, D, labels, K, ws, ws_bytes, samples, out, err_flag);
}
extern "C" int64_t dmvae_mixture_logpdf_ws_bytes(int64_t M, int64_t J, int64_t D) { return mixture_logpdf_ws_bytes(M, J, D); }
extern "C" int dmvae_mixture_logpdf(void* stream, const float* Z, int64_t ldz, int M, int D, const float* mean, int64_t ldm, const float* log_var, int64_t ldv,
                                    int J, const float* log_w, void* ws, int64_t ws_bytes, float* out) {
    return mixture_logpdf_launch((hipStream_t)stream, Z, ldz, M, D, mean, ldm, log_var, ldv, J, log_w, ws, ws_bytes, out);
}
extern "C" int dmvae_mixture_logpdf_split(int M, int J, int D) { return mixture_logpdf_split(M, J, D).nsplit; }
extern "C" int dmvae_posterior_sample(void* stream, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, const float* eps,
                                      int64_t ld_eps, uint64_t seed, uint64_t counter, int64_t pos0, float* Z, int64_t ldz, float* logq) {
    return posterior_sample_launch((hipStream_t)stream, mean, ldm, log_var, ldv, n, D, eps, ld_eps, seed, counter, pos0, Z, ldz, logq);
}
extern "C" int64_t dmvae_column_stats_ws_bytes(int64_t n, int64_t D) { return column_stats_ws_bytes(n, D); }
extern "C" int dmvae_column_stats(void* stream, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, void* ws, int64_t ws_bytes,
                                  double* out) {
    return column_stats_launch((hipStream_t)stream, mean, ldm, log_var, ldv, n, D, ws, ws_bytes, out);
}
extern "C" int dmvae_sum_f64(void* stream, const float* x, int64_t n, double* out) { return sum_f64_launch((hipStream_t)stream, x, n, out); }
extern "C" int64_t dmvae_knn_ws_bytes(int64_t M, int64_t N, int D, int k) { return knn_ws_bytes(M, N, D, k); }
extern "C" int dmvae_knn(void* stream, const float* Q, int64_t ldq, int M, const float* X, int64_t ldx, int N, int D, int k, int64_t self_first, void* ws,
                         int64_t ws_bytes, int32_t* idx, float* d2, int64_t ldo) {
    return knn_launch((hipStream_t)stream, Q, ldq, M, X, ldx, N, D, k, self_first, ws, ws_bytes, idx, d2, ldo);
}
extern "C" int dmvae_knn_vote(void* stream, const int32_t* idx, int64_t ldi, int M, int k, const int32_t* classes, int N, int C, float* counts, int64_t ldc,
                              int32_t* err_flag) {
    return knn_vote_launch((hipStream_t)stream, idx, ldi, M, k, classes, N, C, counts, ldc, err_flag);
}
extern "C" int dmvae_knn_ranks(void* stream, const float* X, int64_t ldx, int N, int D, const int32_t* idx, int64_t ldi, int k, int32_t* ranks, int64_t ldr,
                               int32_t* err_flag) {
    return knn_ranks_launch((hipStream_t)stream, X, ldx, N, D, idx, ldi, k, ranks, ldr, err_flag);
}
extern "C" int dmvae_prdc_counts(void* stream, const float* R, int64_t ldr, int N, const float* F, int64_t ldf, int M, int D, const float* rR2,
                                 const float* rF2, int32_t* fake_in_real, int32_t* real_in_fake, float* real_min_d2, int32_t* real_min_j) {
    return prdc_counts_launch((hipStream_t)stream, R, ldr, N, F, ldf, M, D, rR2, rF2, fake_in_real, real_in_fake, real_min_d2, real_min_j);
}
extern "C" int dmvae_sinkhorn_softmin(void* stream, const float* X, int64_t ldx, int N, const float* Y, int64_t ldy, int M, int D, const float* g,
                                      const float* log_b, float eps, const float* prev, float* out) {
    return sinkhorn_softmin_launch((hipStream_t)stream, X, ldx, N, Y, ldy, M, D, g, log_b, eps, prev, out);
}
extern "C" int dmvae_binarize_rows(void* stream, const float* X, int64_t ldx, int64_t n_rows, int n_cols, int64_t row_base, uint64_t seed, uint64_t counter,
                                   int mode, float* out, int64_t ldo) {
    return binarize_rows_launch((hipStream_t)stream, X, ldx, n_rows, n_cols, row_base, seed, counter, mode, out, ldo);
}
extern "C" int dmvae_augment_rows(void* stream, const float* X, int64_t ldx, int64_t n_rows, int H, int W, int64_t row_base, uint64_t seed, uint64_t counter,
                                  const dmvae_augment_params* p, const float* theta_in, float* theta_out, float* out, int64_t ldo) {
    return augment_rows_launch((hipStream_t)stream, X, ldx, n_rows, H, W, row_base, seed, counter, p, theta_in, theta_out, out, ldo);
}
extern "C" int dmvae_ssim_rows(void* stream, const float* X, int64_t ldx, int64_t nx, const int32_t* ix, const float* Y, int64_t ldy, int64_t ny,
                               const int32_t* iy, int64_t n_pairs, int H, int W, int planes, const float* w1, int win, float c1, float c2, float* ssim,
                               float* sse, int32_t* err_flag) {
    return ssim_rows_launch((hipStream_t)stream, X, ldx, nx, ix, Y, ldy, ny, iy, n_pairs, H, W, planes, w1, win, c1, c2, ssim, sse, err_flag);
}
extern "C" int64_t dmvae_softmax_xent_ws_bytes(int64_t n, int D, int C) { return probe_xent_ws_bytes(n, D, C); }
extern "C" int dmvae_softmax_xent(void* stream, const float* Z, int64_t ldz, int64_t n, int D, const float* shift, const float* scale, const int32_t* classes,
                                  int C, const float* W, int64_t ldw, const float* b, void* ws, int64_t ws_bytes, double* out, int32_t* flag) {
    return probe_xent_launch((hipStream_t)stream, Z, ldz, n, D, shift, scale, classes, C, W, ldw, b, ws, ws_bytes, out, flag);
}
extern "C" int dmvae_linear_scores(void* stream, const float* Z, int64_t ldz, int M, int D, const float* shift, const float* scale, const float* W, int64_t ldw,
                                   const float* b, int C, float* scores, int64_t lds) {
    return probe_scores_launch((hipStream_t)stream, Z, ldz, M, D, shift, scale, W, ldw, b, C, scores, lds);
}
extern "C" int dmvae_graph_sym_normalize(void* stream, const int64_t* indptr, const int32_t* indices, const float* w, int N, int64_t nnz, float* s, float* r,
                                         int32_t* err_flag) {
    return graph_sym_normalize_launch((hipStream_t)stream, indptr, indices, w, N, nnz, s, r, err_flag);
}
extern "C" int64_t dmvae_label_spread_ws_bytes(int64_t N, int C) { return label_spread_ws_bytes(N, C); }
extern "C" int dmvae_label_spread(void* stream, const int64_t* indptr, const int32_t* indices, const float* s, int N, int64_t nnz, const int32_t* labels, int C,
                                  float alpha, int n_iter, const float* F_in, int64_t ld_in, float* F, int64_t ldf, float* change, void* ws,
                                  int64_t ws_bytes, int32_t* err_flag) {
    return label_spread_launch((hipStream_t)stream, indptr, indices, s, N, nnz, labels, C, alpha, n_iter, F_in, ld_in, F, ldf, change, ws, ws_bytes, err_flag);
}
extern "C" int dmvae_recon_nblocks(int B_pad, int I_pad) { return recon_nblocks(B_pad, I_pad); }
extern "C" int dmvae_recon_fwd_bwd(void* stream, int act_dtype, int recon_kind, int B, int B_pad, int I, int I_pad, const float* logits,
                                   int64_t ldl, const float* x, int64_t ldx, float inv_B, void* dl, int64_t ldd, float* partials) {
    DMVAE_REQUIRE(logits && x && dl && partials, "dmvae_recon_fwd_bwd: null pointer");
    DMVAE_REQUIRE(I_pad % 4 == 0 && ldl % 4 == 0 && ldx % 4 == 0 && ldd % 4 == 0 && B <= B_pad && I <= I_pad, "dmvae_recon_fwd_bwd: dims must be multiples of 4");
    return recon_launch((hipStream_t)stream, act_dtype, recon_kind, B, B_pad, I, I_pad, logits, ldl, x, ldx, inv_B, dl, ldd, partials);
}
extern "C" int dmvae_colsum(void* stream, int in_dtype, const void* in, int64_t ld, int M, int N, float* out) {
    DMVAE_REQUIRE(in && out && M > 0 && N > 0, "dmvae_colsum: bad argument");
    if (M > 64) TRY(colsum_prepare(N));   // two-pass path: lazily sized scratch (not capture-safe; plans bring their own)
    return colsum_launch((hipStream_t)stream, in_dtype, in, ld, M, N, out, nullptr, 0);
}
extern "C" int dmvae_loss_finalize(void* stream, const float* rp, int nr, const float* lp, int nl, float inv_B, void* state) {
    DMVAE_REQUIRE(rp && lp && state, "dmvae_loss_finalize: null pointer");
    return loss_finalize_launch((hipStream_t)stream, rp, nr, lp, nl, inv_B, state, 0);
}
extern "C" int dmvae_adam_tf(void* stream, int64_t n, float* param, float* grad, float* m, float* v, void* param_bf16, float lr,
                             float beta1, float beta2, float epsilon, float grad_scale, int flags, uint64_t t_host, const void* state) {
    DMVAE_REQUIRE(param && grad && m && v && n > 0 && n % 4 == 0, "dmvae_adam_tf: n must be a positive multiple of 4");
    DMVAE_REQUIRE(state || t_host >= 1, "dmvae_adam_tf: t starts at 1");
    AdamArgs a;
    a.n = n; a.p = param; a.g = grad; a.m = m; a.v = v; a.pb = reinterpret_cast<bf16_t*>(param_bf16);
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = epsilon; a.gscale = grad_scale; a.zero_grad = (flags & DMVAE_ADAM_ZERO_GRAD) != 0; a.ieee = (flags & DMVAE_ADAM_IEEE) != 0;
    a.t_host = t_host; a.st = reinterpret_cast<const dmvae_state*>(state);
    if (flags & DMVAE_ADAM_SHADOW) return adam_shadow_launch((hipStream_t)stream, a, (flags >> 8) & 0xffff);
    return adam_launch((hipStream_t)stream, a);
}
extern "C" int dmvae_adam_finish(void* stream, void* state) {
    DMVAE_REQUIRE(state, "dmvae_adam_finish: null state");
    return adam_finish_launch((hipStream_t)stream, state);
}
extern "C" int dmvae_gather_rows(void* stream, int act_dtype, const float* data, int64_t n_rows, int dim, const int32_t* perm,
                                 int64_t first, int batch, int n_valid, int B_pad, void* out_act, int64_t ld_act, float* out_f32,
                                 int64_t ld_f32, const void* state) {
    DMVAE_REQUIRE(data && (out_act || out_f32), "dmvae_gather_rows: null pointer");
    const int64_t ld = out_act ? ld_act : ld_f32;
    DMVAE_REQUIRE(ld % 4 == 0 && ld >= dim && (!out_act || !out_f32 || ld_act == ld_f32), "dmvae_gather_rows: ld must be a multiple of 4, >= dim, equal for both outputs");
    return gather_launch((hipStream_t)stream, act_dtype, data, n_rows, dim, perm, first, batch, n_valid, B_pad, out_act, ld_act, out_f32, ld_f32, (int)ld, state);
}
extern "C" int dmvae_philox_normal(void* stream, float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t sid) {
    DMVAE_REQUIRE(out && n > 0, "dmvae_philox_normal: bad argument");
    return philox_launch((hipStream_t)stream, out, n, seed, step, sid, 0);
}
extern "C" int dmvae_philox_uniform(void* stream, float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t sid) {
    DMVAE_REQUIRE(out && n > 0, "dmvae_philox_uniform: bad argument");
    return philox_launch((hipStream_t)stream, out, n, seed, step, sid, 2);
}
extern "C" int dmvae_philox_gumbel(void* stream, float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t sid) {
    DMVAE_REQUIRE(out && n > 0, "dmvae_philox_gumbel: bad argument");
    return philox_launch((hipStream_t)stream, out, n, seed, step, sid, 1);
}
extern "C" int dmvae_cast_f32_to_bf16(void* stream, const float* in, void* out, int64_t n) {
    DMVAE_REQUIRE(in && out && n > 0, "dmvae_cast: bad argument");
    return cast_launch((hipStream_t)stream, in, out, n, 1);
}
extern "C" int dmvae_cast_bf16_to_f32(void* stream, const void* in, float* out, int64_t n) {
    DMVAE_REQUIRE(in && out && n > 0, "dmvae_cast: bad argument");
    return cast_launch((hipStream_t)stream, in, out, n, 0);
}

extern "C" int dmvae_debug_spin(void* stream, int microseconds) { return spin_launch((hipStream_t)stream, microseconds); }
extern "C" int dmvae_debug_strip_fwd2(void* stream, int B_pad, int K0, const void* X, int64_t ldx, const void* W0, int64_t ld0, const float* b0,
                                      const void* W1, int64_t ld1, const float* b1, void* Y1, int64_t ldy1, void* Y2, int64_t ldy2) {
    return strip_fwd2_launch((hipStream_t)stream, B_pad, K0, X, ldx, W0, ld0, b0, W1, ld1, b1, Y1, ldy1, Y2, ldy2);
}
extern "C" int dmvae_debug_stamps(void** device_ptr) {
    if (!device_ptr) return DMVAE_EINVAL;
    *device_ptr = gemm_bf16_stamps();
    if (!*device_ptr) *device_ptr = heads_dx_phase_table();      // measurement build 10: the phase table of heads_dx.hip (measure.h)
    return *device_ptr ? 0 : DMVAE_ESTATE;
}

extern "C" int dmvae_debug_anatomy(void** device_ptr) {
    if (!device_ptr) return DMVAE_EINVAL;
    *device_ptr = gemm_bf16_anatomy();
    return *device_ptr ? 0 : DMVAE_ESTATE;
}
extern "C" int dmvae_debug_anatomy256(void** device_ptr) {
    if (!device_ptr) return DMVAE_EINVAL;
    *device_ptr = gemm_bf16_256_anatomy();
    return *device_ptr ? 0 : DMVAE_ESTATE;
}

// ---- the CNN trunk's kernels on caller-owned buffers (tests/test_gpu_conv_kernels.py): thin wrappers over the launchers of conv.hip
extern "C" int dmvae_debug_conv_first_fwd(void* stream, int dtype, const void* x, int64_t bstride, int H, int64_t n_img, const void* W, int ldw,
                                          const float* bias, void* out, int ld) {
    DMVAE_REQUIRE((dtype == DMVAE_F32 || dtype == DMVAE_BF16) && x && W && bias && out && H > 0 && n_img > 0 && bstride >= (int64_t)H * H, "dmvae_debug_conv_first_fwd: bad argument");
    return conv_first_fwd_launch((hipStream_t)stream, dtype, x, bstride, H, n_img, W, ldw, bias, 32, out, ld);
}
extern "C" int dmvae_debug_conv_first_dw(void* stream, int dtype, const void* x, int64_t bstride, int H, int64_t n_img, const void* dY, int ld,
                                         float* dW, int ldw, float* db, float* part, int64_t part_floats, int* n_blocks) {
    DMVAE_REQUIRE((dtype == DMVAE_F32 || dtype == DMVAE_BF16) && H > 0 && H % 4 == 0 && n_img > 0 && (ld == 32 || ld == 64) && n_blocks &&
                  n_img * H * (H / 4) < (1ll << 31), "dmvae_debug_conv_first_dw: bad argument (side a multiple of 4, ld 32 or 64)");      // what the launcher takes: the size query answers for nothing else
    *n_blocks = conv_first_dw_blocks(H, n_img);
    if (!part) return 0;                       // size query
    DMVAE_REQUIRE(x && dY && dW && db && bstride >= (int64_t)H * H && part_floats >= (int64_t)*n_blocks * 320,
                  "dmvae_debug_conv_first_dw: bad argument (scratch: %d blocks x 320 floats)", *n_blocks);
    return conv_first_dw_launch((hipStream_t)stream, dtype, x, bstride, H, n_img, dY, ld, 32, dW, ldw, db, part);
}
extern "C" int dmvae_debug_zero_border(void* stream, int dtype, void* a, int P, int ld, int64_t n_img) {
    DMVAE_REQUIRE((dtype == DMVAE_F32 || dtype == DMVAE_BF16) && a && P >= 2 && n_img > 0, "dmvae_debug_zero_border: bad argument");
    return zero_border_launch((hipStream_t)stream, dtype, a, P, ld, n_img);
}
extern "C" int dmvae_debug_maxpool2_fwd(void* stream, int dtype, const void* in, int H, int ld, int64_t n_img, void* out, int out_border) {
    DMVAE_REQUIRE((dtype == DMVAE_F32 || dtype == DMVAE_BF16) && in && out && H > 0 && n_img > 0 && (out_border == 0 || out_border == 1), "dmvae_debug_maxpool2_fwd: bad argument");
    return maxpool2_fwd_launch((hipStream_t)stream, dtype, in, H, ld, n_img, out, out_border);
}
extern "C" int dmvae_debug_maxpool2_bwd_relu(void* stream, int dtype, const void* in, const void* dout, int H, int ld, int64_t n_img, void* din, int dout_border) {
    DMVAE_REQUIRE((dtype == DMVAE_F32 || dtype == DMVAE_BF16) && in && dout && din && H > 0 && n_img > 0 && (dout_border == 0 || dout_border == 1), "dmvae_debug_maxpool2_bwd_relu: bad argument");
    return maxpool2_bwd_relu_launch((hipStream_t)stream, dtype, in, dout, H, ld, n_img, din, dout_border);
}
extern "C" int dmvae_debug_conv_wflip(void* stream, int dtype, const void* W, int cin, int cin_ld, int cout, int ldw, void* Wt, int Kt) {
    DMVAE_REQUIRE((dtype == DMVAE_F32 || dtype == DMVAE_BF16) && W && Wt && cin > 0 && cout > 0 && ldw >= cout, "dmvae_debug_conv_wflip: bad argument");
    return conv_wflip_launch((hipStream_t)stream, dtype, W, cin, cin_ld, cout, ldw, Wt, Kt);
}
extern "C" int dmvae_debug_conv_gemm(void* stream, int dtype, int layout, int M, int N, int K, const void* A, int64_t lda,
                                     const void* B, int64_t ldb, const dmvae_epilogue* epi, int split_k, int conv_p, int conv_c) {
    DMVAE_REQUIRE(conv_p >= 3 && conv_c > 0, "dmvae_debug_conv_gemm: conv_p = side + 2 >= 3, conv_c > 0");
    return gemm_checked((hipStream_t)stream, dtype, layout, M, N, K, A, lda, B, ldb, epi, split_k, nullptr, conv_p, conv_c);
}
extern "C" int dmvae_debug_conv_dw(void* stream, int dtype, int rows, int conv_p, int conv_c, const void* X, int64_t ldx, const void* dY, int64_t ldy,
                                   int N, int n_valid, int split, float* slab, float* dW, float* db) {
    DMVAE_REQUIRE(rows > 0 && conv_p >= 3 && conv_c > 0 && N > 0 && n_valid > 0 && n_valid <= N && dW && db && split >= 1 && rows % (split * 64) == 0 && (split == 1 || slab),
                  "dmvae_debug_conv_dw: bad argument");
    const int kdim = pad64(9 * conv_c);
    hipError_t me = hipMemsetAsync(dW, 0, (size_t)kdim * N * 4, (hipStream_t)stream);      // (the plan zeroes its whole conv gradient range up front)
    if (me == hipSuccess) me = hipMemsetAsync(db, 0, (size_t)N * 4, (hipStream_t)stream);
    if (me != hipSuccess) { set_error("dmvae_debug_conv_dw memset: %s", hipGetErrorString(me)); return (int)me; }
    return conv_layer_dw((hipStream_t)stream, dtype, rows, conv_p, conv_c, kdim, X, ldx, dY, ldy, N, n_valid, split, slab, dW, db);
}

// ---- step_finalize and the rider launches on caller-owned buffers (tests/test_gpu_step_finalize.py): thin wrappers over the launchers the pass uses
static int debug_finalize_args(const dmvae_debug_finalize* f, const char* who, dmvae_finalize_args* out) {
    DMVAE_REQUIRE(f && f->rp && f->lp && f->state && f->nr >= 0 && f->nl >= 0 && f->nblk >= 0 && f->ncol >= 0 && (f->ncol == 0 || (f->part && f->gout)),
                  "%s: step_finalize arguments: null pointer or negative count", who);
    *out = step_finalize_args(f->rp, f->nr, f->lp, f->nl, f->inv_B, f->state, f->bump_adam, f->b1, f->b2, f->part, f->nblk, f->ncol, f->gout);
    return 0;
}
extern "C" int dmvae_debug_step_finalize(void* stream, const dmvae_debug_finalize* fin) {
    dmvae_finalize_args f;
    TRY(debug_finalize_args(fin, "dmvae_debug_step_finalize", &f));
    return step_finalize_launch((hipStream_t)stream, f.rp, f.nr, f.lp, f.nl, f.inv_B, f.st, f.bump_adam, f.b1, f.b2, f.part, f.nblk, f.ncol, f.gout);
}
extern "C" int dmvae_debug_gemm_dx_riders(void* stream, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, const dmvae_epilogue* epi,
                                          const dmvae_debug_finalize* fin, const dmvae_debug_gather* gat, int ngat, int gat_last) {
    DMVAE_REQUIRE(epi && (epi->kind == DMVAE_EPI_LATENT || epi->kind == DMVAE_EPI_RELU_MASK), "dmvae_debug_gemm_dx_riders: the LATENT or RELU_MASK epilogue");
    DMVAE_REQUIRE(fin || gat, "dmvae_debug_gemm_dx_riders: no riders (use dmvae_gemm)");
    DMVAE_REQUIRE(gat ? (ngat > 0 && ngat % 8 == 0) : ngat == 0, "dmvae_debug_gemm_dx_riders: ngat=%d: a positive multiple of 8 with a gather, 0 without", ngat);
    DMVAE_REQUIRE(!(fin && gat && gat->state), "dmvae_debug_gemm_dx_riders: step_finalize advances the batch cursor a gather addressed through the state reads: not in one launch");
    GemmArgs a;
    TRY(gemm_checked((hipStream_t)stream, DMVAE_BF16, DMVAE_GEMM_DX, M, N, K, A, lda, B, ldb, epi, 1, &a));
    GemmRiders r{};
    if (fin) {
        TRY(debug_finalize_args(fin, "dmvae_debug_gemm_dx_riders", &r.fin));
        r.nfin = (r.fin.nblocks + 7) & ~7;
    }
    if (gat) {
        DMVAE_REQUIRE(gat->data && gat->out_bf16 && gat->n_rows >= 0 && gat->dim > 0 && gat->B_pad > 0 && gat->n_valid >= 0 && gat->n_valid <= gat->B_pad &&
                      gat->ld % 4 == 0 && gat->ld >= gat->dim && (int64_t)gat->B_pad * (gat->ld / 4) < (int64_t(1) << 31) - int64_t(512) * 512 * 16,
                      "dmvae_debug_gemm_dx_riders: gather arguments (ld a multiple of 4, >= dim; n_valid <= B_pad; B_pad x ld within 32-bit quad indices)");
        r.gat = gather_args(DMVAE_BF16, gat->data, gat->n_rows, gat->dim, gat->perm, gat->first, gat->batch, gat->n_valid, gat->B_pad, gat->out_bf16, gat->ld,
                            nullptr, gat->ld, (int)gat->ld, gat->state);
        r.ngat = ngat;
        r.gat_last = gat_last ? 1 : 0;
    }
    DMVAE_REQUIRE(gemm_bf16_riders_room(a, false) >= r.nfin + r.ngat, "dmvae_debug_gemm_dx_riders: %d rider ids, the launch has room for %d (-1: not a small-tile launch)",
                  r.nfin + r.ngat, gemm_bf16_riders_room(a, false));
    DMVAE_REQUIRE(!fin || gemm_bf16_carries_finalize(a), "dmvae_debug_gemm_dx_riders: the two-wave 16-row tile cannot carry the step_finalize blocks");
    return gemm_bf16_dispatch((hipStream_t)stream, DMVAE_GEMM_DX, a, 1, &r);
}
extern "C" int dmvae_debug_gemm_grouped_fin(void* stream, const dmvae_gemm_problem* probs, int n, const dmvae_debug_finalize* fin) {
    DMVAE_REQUIRE(probs && n >= 1 && n <= DMVAE_MAX_GROUP, "dmvae_debug_gemm_grouped_fin: 1..%d problems", DMVAE_MAX_GROUP);
    dmvae_finalize_args f;
    TRY(debug_finalize_args(fin, "dmvae_debug_gemm_grouped_fin", &f));
    hipStream_t s = (hipStream_t)stream;
    std::vector<GemmArgs> q(n);
    for (int i = 0; i < n; ++i) {
        const dmvae_gemm_problem& pr = probs[i];
        TRY(gemm_checked(s, DMVAE_BF16, DMVAE_GEMM_DX, pr.M, pr.N, pr.K, pr.A, pr.lda, pr.B, pr.ldb, &pr.epi, 1, &q[i]));
    }
    return gemm_bf16_grouped(s, DMVAE_GEMM_DX, q.data(), n, &f);
}

// ---- the 256x256 macro tile with the arguments only the step sets (tests/test_gpu_gemm256_forms.py): column sums out / in, K slices into slabs
extern "C" int dmvae_debug_gemm256(void* stream, int layout, const dmvae_debug_gemm256_problem* probs, int n, const dmvae_adam_ctx* ctx) {
    DMVAE_REQUIRE(probs && n >= 1 && n <= DMVAE_MAX_GROUP, "dmvae_debug_gemm256: 1..%d problems", DMVAE_MAX_GROUP);
    DMVAE_REQUIRE(layout >= 0 && layout <= 2, "dmvae_debug_gemm256: bad layout %d", layout);
    DMVAE_REQUIRE(layout == DMVAE_GEMM_DW || n == 1, "dmvae_debug_gemm256: the FWD and DX layouts take one problem (%d given)", n);
    hipStream_t s = (hipStream_t)stream;
    std::vector<GemmArgs> q(n);
    bool adam = false;
    for (int i = 0; i < n; ++i) {
        const dmvae_debug_gemm256_problem& d = probs[i];
        const dmvae_gemm_problem& pr = d.p;
        DMVAE_REQUIRE(pr.epi.recon_kind == 0 || pr.epi.recon_kind == 1, "dmvae_debug_gemm256: recon_kind %d (0 binary, 1 real)", pr.epi.recon_kind);
        GemmArgs& a = q[i];
        TRY(gemm_checked(s, DMVAE_BF16, layout, pr.M, pr.N, pr.K, pr.A, pr.lda, pr.B, pr.ldb, &pr.epi, 1, &a));
        const int epi = pr.epi.kind;
        if (!gemm_bf16_256_instantiated(layout, epi)) {
            set_error("dmvae_debug_gemm256: layout %d with epilogue %d is not instantiated on the macro tile", layout, epi);
            return DMVAE_EUNSUPPORTED;
        }
        DMVAE_REQUIRE(pr.M % 256 == 0 && pr.N % 256 == 0, "dmvae_debug_gemm256: M=%d N=%d must be multiples of 256", pr.M, pr.N);
        const bool sums_out = (layout == DMVAE_GEMM_FWD && epi == DMVAE_EPI_BIAS_RECON) || (layout == DMVAE_GEMM_DX && epi == DMVAE_EPI_RELU_MASK);
        DMVAE_REQUIRE(!d.csum_out || (sums_out && d.csum_ld >= pr.N && d.csum_ld % 4 == 0 && (uintptr_t)d.csum_out % 16 == 0),
                      "dmvae_debug_gemm256: csum_out goes with FWD + BIAS_RECON / DX + RELU_MASK, 16-byte aligned, csum_ld >= N a multiple of 4");
        DMVAE_REQUIRE(!d.csum_in || (layout == DMVAE_GEMM_DW && pr.epi.out2 && d.csum_rows >= 1 && (uintptr_t)d.csum_in % 16 == 0),
                      "dmvae_debug_gemm256: csum_in goes with a DW problem that has a bias gradient (epi.out2), 16-byte aligned, csum_rows >= 1");
        DMVAE_REQUIRE(!(d.csum_in && d.csum_out), "dmvae_debug_gemm256: csum_out and csum_in in one problem");
        DMVAE_REQUIRE(d.k_split == 0 || d.k_split == pr.K || (layout == DMVAE_GEMM_DW && d.k_split > 0 && d.k_split % 64 == 0 && pr.K % d.k_split == 0),
                      "dmvae_debug_gemm256: k_split=%d: DW layout only, a multiple of 64 that divides K=%d (0: no slices)", d.k_split, pr.K);
        DMVAE_REQUIRE(d.slab_stride >= 0, "dmvae_debug_gemm256: negative slab_stride");
        a.csum_out = d.csum_out; a.csum_in = d.csum_in; a.csum_ld = d.csum_ld; a.csum_rows = d.csum_rows;
        if (d.k_split > 0) a.k_split = d.k_split;
        a.slab_stride = d.slab_stride;
        adam = adam || epi == DMVAE_EPI_ADAM;
    }
    if (adam) {      // what dmvae_gemm_grouped_dw_adam asks of its context (the segment stays with the grouped launch: none here)
        DMVAE_REQUIRE(ctx && ctx->param && ctx->grad && ctx->m && ctx->v && ctx->state && ctx->seg_n == 0, "dmvae_debug_gemm256: DMVAE_EPI_ADAM needs a context with its arenas and state, and no extra segment");
        for (int i = 0; i < n; ++i) {
            DMVAE_REQUIRE(q[i].epi.kind == DMVAE_EPI_ADAM, "dmvae_debug_gemm256: one call is all DMVAE_EPI_ADAM or none");
            const int64_t end = (reinterpret_cast<const float*>(q[i].epi.out) - ctx->grad) + (int64_t)q[i].M * q[i].epi.ldo;
            if (end < 0 || end > (int64_t(1) << 30)) { set_error("dmvae_debug_gemm256: gradient %d ends %lld elements into the arena (limit 2^30)", i, (long long)end); return DMVAE_EUNSUPPORTED; }
        }
    }
    if (layout != DMVAE_GEMM_DW) return gemm_bf16_256_launch(s, layout, q[0], nullptr);
    return gemm_bf16_256_dw_all(s, q.data(), n, adam ? ctx : nullptr);
}

extern "C" int dmvae_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return 0;
}
extern "C" int dmvae_prof_collect(dmvae_prof_row* rows, int max_rows) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    std::map<std::string, dmvae_prof_row> agg;
    std::vector<std::string> order;
    for (auto& r : g_prof) {
        (void)hipEventSynchronize(r.e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        // the kernels' own durations: per dispatch, stop - start of the pair hipExtLaunchKernelGGL bound to it
        double kms = 0.0;
        bool kok = !r.k.empty();
        for (auto& pr : r.k) {
            float d = 0.f;
            if (hipEventSynchronize(pr.second) != hipSuccess || hipEventElapsedTime(&d, pr.first, pr.second) != hipSuccess || !(d > 0.f)) kok = false;
            kms += d;
            g_event_pool.push_back(pr.first);
            g_event_pool.push_back(pr.second);
        }
        (void)hipGetLastError();
        auto it = agg.find(r.name);
        if (it == agg.end()) {
            dmvae_prof_row row;
            memset(&row, 0, sizeof(row));
            snprintf(row.name, sizeof(row.name), "%s", r.name);
            it = agg.emplace(r.name, row).first;
            order.push_back(r.name);
        }
        it->second.launches += 1;
        it->second.total_ms += ms;
        it->second.kernel_ms += kok ? kms : 0.0;
        it->second.kernel_launches += kok ? (int64_t)r.k.size() : 0;
        it->second.flops += r.flops;
        it->second.bytes += r.bytes;
        g_event_pool.push_back(r.e0);
        g_event_pool.push_back(r.e1);
    }
    g_prof.clear();
    g_prof_cur = -1;
    int n = 0;
    for (auto& k : order) {
        if (n >= max_rows) break;
        rows[n++] = agg[k];
    }
    return n;
}

extern "C" int dmvae_debug_set_tile(int bm, int bn) {
    DMVAE_REQUIRE((bm == 0 && bn == 0) || ((bm == 64 || bm == 128) && (bn == 64 || bn == 128)), "dmvae_debug_set_tile: 64 or 128 (0,0 = heuristic)");
    gemm_bf16_force_tile(bm * 1000 + bn);
    return 0;
}

extern "C" int dmvae_debug_set_knob(int which, int value) {
    if (step_set_knob(which, value)) return 0;      // 10, 11, 12, 16, 17, 21: the pass's own (step.hip)
    if (which == 13) { heads_dx_stream_set(value); return 0; }
    if (which == 18 || which == 20) { gemm_bf16_set_knob(which, value); return 0; }
    if (which == 19) { heads_latent_set(value); return 0; }
    if (which == 22) { latent_vade_force_mfma(value); return 0; }
    if (which == 14) { latent_set_blocks_target(value); return 0; }      // (the block count in use is taken at enqueue time and checked against the plan's capacity)
    DMVAE_REQUIRE(which >= 0 && which <= 9 && which != 3, "dmvae_debug_set_knob: knob 0 = supertile rows, 1 = 8-wave workgroups, 2 = per-problem tiles in grouped grids, (3: removed, the deep-ring policy), 4 = XCD runs per tile class in grouped grids, 5 = short-K conv tiles, 6 = 256x256 tile policy, 7 = short-K workgroups, 8 = first-tile stagger of the merged dW grid, 9 = waves per workgroup of a grouped dX launch; 10 / 11 = K slices of the dW groups, 12 = heads dX as one or two launches, 13 = heads dX on the streaming kernel (1) or the grouped tiles (0), 14 = blocks the latent kernel's geometry aims at (512), 19 = fused heads + latent launch, 20 = XCD partition of the grouped dW launch, 21 = K slices of a small batch's thin launches, 22 = VaDE's large-table latent form wherever the caller brings its scratch");
    gemm_bf16_set_knob(which, value);
    return 0;
}

extern "C" int dmvae_abi_version(void) { return DMVAE_ABI_VERSION; }
extern "C" const char* dmvae_last_error(void) { return g_err; }
