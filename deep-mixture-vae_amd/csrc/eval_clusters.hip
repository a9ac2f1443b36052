// Clustering evaluation on the device: what get_accuracy needs of a batch is one integer per row -- the arg-max of its
// scores -- counted against the row's class (get_clustering_accuracy, includes/utils.py:22-34 of the reference: the
// [cluster][class] confusion matrix that the Hungarian step is solved on).  Two row kernels of the latent_vade.hip /
// moe_head.hip family, 16 lanes per row, 16 rows per 256-thread workgroup:
//
//   confusion_add_kernel   scores [n][K] f32 (DMVAE / MoE: the logits) -> cluster = first index of the row's largest
//                          score (np.argmax's rule), conf[cluster][class] += 1.
//   vade_eval_kernel       VaDE (base_models.py:654-670): from the encoder's mean / log_var, for the draws j < k in
//                          ascending order  Z_j = mean + exp(log_var / 2) eps_j,  gamma_j = get_cluster_probs(Z_j)
//                          (priors.py:91-102; the formula is in the header of latent_vade.hip),  w = (sum_j gamma_j) / k,
//                          written out, then the same arg-max and count on w.  The prior tables are whole in LDS as
//                          latent_vade_kernel holds them; tables past its 60 KiB take the per-draw forward half of
//                          latent_vade_mfma.hip (vade_eval_mfma_launch), then confusion_add_kernel on w.
//                          eps_j: the caller's buffer [k][n][ld_eps], or Philox keyed by
//                          (seed, counter, stream EVAL_PHILOX_STREAM, element ((j * n_rows + first + r) * D + d)): the
//                          noise of a row depends on its POSITION in the evaluated order, not on the batch size.
//
// The class of batch row r is classes[perm ? perm[first + r] : first + r] -- the indexing of the batch gather.  Counts
// are integers: the one global integer atomic per row is exact in any order, so the matrix is reproducible (the
// project's rule is no FLOAT atomics).  A class outside [0, R) or a permutation entry outside [0, n_rows) counts
// nothing and sets a bit of the error flag.  Rows >= n_valid count nothing and are not launched.
#include "latent_body.h"
#include "eval_clusters.h"
#include "row_argmax.h"

namespace dmvae {

constexpr int EVAL_RB = 16;        // rows per workgroup

// (row_argmax16: row_argmax.h)

// one lane per row; 0 <= first and first + n_valid <= n_rows were checked on the host, cluster < K <= R
__device__ __forceinline__ void eval_count(const EvalRows& r, int b, int cluster) {
    const int64_t i = r.first + b;
    const int64_t src = r.perm ? (int64_t)r.perm[i] : i;
    if (src < 0 || src >= r.n_rows) { atomicOr(r.err_flag, EVAL_ERR_PERM); return; }
    const int c = r.classes[src];
    if (c < 0 || c >= r.R) { atomicOr(r.err_flag, EVAL_ERR_CLASS); return; }
    atomicAdd(r.conf + (int64_t)cluster * r.R + c, 1);
}

__global__ __launch_bounds__(256) void confusion_add_kernel(const float* scores, int64_t ld, int K, EvalRows r) {
    const int lane = threadIdx.x & 15;
    const int b = blockIdx.x * EVAL_RB + (threadIdx.x >> 4);
    const bool valid = b < r.n_valid;
    const int bi = row_argmax16(scores + (int64_t)(valid ? b : 0) * ld, valid ? K : 0, lane);
    if (valid && lane == 0) eval_count(r, b, bi);
}

__global__ __launch_bounds__(256) void vade_eval_kernel(VadeEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = a.K, D = a.D, DP = D + 1;
    constexpr int RB = EVAL_RB;
    float* tpm = lds;                 // [K][DP] prior means
    float* tip = tpm + K * DP;        // [K][DP] exp(-prior_log_var)
    float* ck = tip + K * DP;         // [K] sum_d prior_log_var
    float* us = ck + K;               // [RB][K] u, then exp(u - max) of the current draw
    float* wacc = us + RB * K;        // [RB][K] sum_j gamma_j
    float* rz = wacc + RB * K;        // [RB][DP] z of the current draw
    float* rmu = rz + RB * DP;        // [RB][DP] mean
    float* rsd = rmu + RB * DP;       // [RB][DP] exp(log_var / 2)

    const int tid = threadIdx.x, lr = tid & 15, rsub = tid >> 4;
    const int b = blockIdx.x * RB + rsub;
    const bool valid = b < a.rows.n_valid;

    for (int idx = tid; idx < K * D; idx += 256) {
        const int k = idx / D, d = idx - k * D;
        tpm[k * DP + d] = a.prior_means[idx];
        tip[k * DP + d] = __expf(-a.prior_log_vars[idx]);
    }
    for (int k = rsub; k < K; k += 16) {          // as latent_vade_kernel sums them: the same c_k bits
        float s = 0.f;
        for (int d0 = lr; d0 < D; d0 += 64) {
            float t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = d0 + 16 * i;
                t[i] = a.prior_log_vars[(int64_t)k * D + (d < D ? d : 0)];
                t[i] = d < D ? t[i] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) s += t[i];
        }
        s = row_sum16(s);
        if (lr == 0) ck[k] = s;
    }
    for (int d = lr; d < D; d += 16) {            // lane owns d = lr + 16 i
        float mu = 0.f, sd = 0.f;
        if (valid) {
            mu = a.mean[(int64_t)b * a.ld_mean + d];
            sd = __expf(0.5f * a.log_var[(int64_t)b * a.ld_log_var + d]);
        }
        rmu[rsub * DP + d] = mu;
        rsd[rsub * DP + d] = sd;
    }
    for (int k = lr; k < K; k += 16) wacc[rsub * K + k] = 0.f;      // lane owns k = lr + 16 i (nobody else touches them)

    const uint64_t pos = (uint64_t)(a.rows.first + b);
    for (int j = 0; j < a.draws; ++j) {
        for (int d = lr; d < D; d += 16) {
            float ep = 0.f;
            if (valid)
                ep = a.eps ? a.eps[((int64_t)j * a.rows.n_valid + b) * a.ld_eps + d]
                           : philox_normal_at(a.seed, a.counter, EVAL_PHILOX_STREAM, ((uint64_t)j * (uint64_t)a.rows.n_rows + pos) * (uint64_t)D + d);
            rz[rsub * DP + d] = rmu[rsub * DP + d] + rsd[rsub * DP + d] * ep;
        }
        __syncthreads();                          // z of this draw (first draw: the tables too)
        float mx = -INFINITY;
        for (int k = lr; k < K; k += 16) {
            float su = 0.f;
            for (int d = 0; d < D; ++d) {
                const float dz = rz[rsub * DP + d] - tpm[k * DP + d];
                su += dz * dz * tip[k * DP + d];
            }
            const float u = -0.5f * (su + ck[k]);
            us[rsub * K + k] = u;
            mx = fmaxf(mx, u);
        }
        mx = row_max16(mx);
        float se = 0.f;
        for (int k = lr; k < K; k += 16) {
            const float ex = __expf(us[rsub * K + k] - mx);
            us[rsub * K + k] = ex;
            se += ex;
        }
        se = row_sum16(se);
        for (int k = lr; k < K; k += 16) wacc[rsub * K + k] += us[rsub * K + k] / se;
        __syncthreads();                          // the next draw overwrites z
    }
    const float nd = (float)a.draws;
    for (int k = lr; k < K; k += 16) {
        const float w = wacc[rsub * K + k] / nd;
        wacc[rsub * K + k] = w;
        if (valid) a.w[(int64_t)b * a.ld_w + k] = w;
    }
    const int bi = row_argmax16(wacc + rsub * K, valid ? K : 0, lr);      // every lane reads back its own entries only
    if (valid && lr == 0) eval_count(a.rows, b, bi);
}

static size_t vade_eval_lds_bytes(int D, int K) {
    return sizeof(float) * ((size_t)2 * K * (D + 1) + K + (size_t)2 * EVAL_RB * K + (size_t)3 * EVAL_RB * (D + 1));
}
#define EVAL_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int eval_rows_check(const EvalRows& r, int K, const char* who) {
    EVAL_REQUIRE(r.classes && r.conf && r.err_flag, "%s: null classes / conf / err_flag", who);
    EVAL_REQUIRE(K >= 1 && r.R >= K && r.R <= EVAL_MAX_R, "%s: K=%d, R=%d (1 <= K <= R <= %d)", who, K, r.R, EVAL_MAX_R);
    EVAL_REQUIRE(r.n_valid >= 0 && r.first >= 0 && r.first + r.n_valid <= r.n_rows,
                 "%s: rows [%lld, %lld + %d) are not inside the %lld rows of classes / perm", who, (long long)r.first, (long long)r.first, r.n_valid,
                 (long long)r.n_rows);
    return 0;
}

int vade_eval_check(const VadeEvalArgs& a, const char* who) {
    if (int rc = eval_rows_check(a.rows, a.K, who)) return rc;
    EVAL_REQUIRE(a.D >= 1 && a.mean && a.log_var && a.prior_means && a.prior_log_vars && a.w, "%s: null pointer / D=%d", who, a.D);
    EVAL_REQUIRE(a.draws >= 1 && a.draws <= EVAL_MAX_DRAWS, "%s: draws=%d (1 .. %d)", who, a.draws, EVAL_MAX_DRAWS);
    EVAL_REQUIRE(a.ld_mean >= a.D && a.ld_log_var >= a.D && a.ld_w >= a.K && (!a.eps || a.ld_eps >= a.D), "%s: leading dimension too small", who);
    if (latent_vade_mfma_needed(a.D, a.K)) {          // the limit of the step's one-kernel form is the limit of vade_eval_kernel
        const int64_t need = a.B_pad > 0 && a.B_pad % 64 == 0 ? latent_vade_mfma_ws_bytes(a.B_pad, a.D, a.K, nullptr) : 0;
        EVAL_REQUIRE(need > 0 && a.B_pad >= a.rows.n_valid && a.ws && a.ws_bytes >= need,
                     "%s (VaDE): K=%d D=%d takes the large-table form, which needs %lld bytes of scratch for B_pad=%d rows (a multiple of 64, >= n_valid=%d)",
                     who, a.K, a.D, (long long)need, a.B_pad, a.rows.n_valid);
    }
    return 0;
}

int confusion_add_launch(hipStream_t s, const float* scores, int64_t ld, int K, const EvalRows& r) {
    if (int rc = eval_rows_check(r, K, "dmvae_confusion_add")) return rc;
    EVAL_REQUIRE(scores && ld >= K, "dmvae_confusion_add: null scores / ld=%lld < K=%d", (long long)ld, K);
    if (r.n_valid == 0) return 0;
    const int nblk = (r.n_valid + EVAL_RB - 1) / EVAL_RB;
    ProfScope ps(s, "confusion_add", (double)r.n_valid * K, 4.0 * r.n_valid * (K + 3.0));
    DMVAE_LAUNCH(confusion_add_kernel, dim3(nblk), dim3(256), 0, s, scores, ld, K, r);
    return check_launch("confusion_add");
}

int vade_eval_launch(hipStream_t s, const VadeEvalArgs& a) {
    if (int rc = vade_eval_check(a, "dmvae_plan_eval_clusters")) return rc;
    if (a.rows.n_valid == 0) return 0;
    if (latent_vade_mfma_needed(a.D, a.K)) return vade_eval_mfma_launch(s, a);
    const int nblk = (a.rows.n_valid + EVAL_RB - 1) / EVAL_RB;
    const double n = a.rows.n_valid;
    ProfScope ps(s, "vade_eval", 3.0 * n * a.draws * (double)a.K * a.D,
                 4.0 * (n * (2.0 * a.D + a.K + 3.0 + (a.eps ? (double)a.draws * a.D : 0.0)) + 2.0 * a.K * a.D * nblk));
    DMVAE_LAUNCH(vade_eval_kernel, dim3(nblk), dim3(256), vade_eval_lds_bytes(a.D, a.K), s, a);
    return check_launch("vade_eval");
}

}  // namespace dmvae
