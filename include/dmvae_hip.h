/*
 * dmvae_hip.h -- C ABI of the MI355X (gfx950) DMVAE training-step library.
 *
 * This is the drop-in boundary for the ONE hot path of ffs97/deep-mixture-vae:
 * everything that the reference executes inside
 *     session.run([self.loss, self.train_step], feed_dict)      code/base_models.py:126-129
 * (forward MLPs, reparameterisation, mixture KL, Bernoulli reconstruction
 * loss, autodiff backward, Adam) plus the host batch assembly that feeds it.
 * The reference has no FFI of its own (pure Python over TensorFlow 1.x), so
 * each entry point names the TensorFlow op / reference line it replaces.
 * Behind the step: evaluation on the device -- clustering accuracy, log-likelihood, t-SNE, and the label-free
 * and contingency cluster metrics' device half (dmvae_argmax_labels, dmvae_silhouette).
 *
 * Conventions
 *   - plain C: device pointers + sizes, no C++ / torch types.
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work
 *     on it (safe under stream capture); nothing synchronises or allocates.
 *   - every function returns 0 on success, a negative DMVAE_E* code for an
 *     argument error, or a positive hipError_t; dmvae_last_error() gives text.
 *   - matrices are row-major with an explicit leading dimension (elements).
 *   - "act" buffers are bf16 when dtype == DMVAE_BF16, float when DMVAE_F32.
 *   - not re-entrant on the same stream/plan; distinct streams are independent.
 */
#ifndef DMVAE_HIP_H
#define DMVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: dmvae_buffers.arena_elems, dmvae_config.model, dmvae_latent_args.mfma_ws(_bytes), dmvae_config.adam_ieee and
 *    dmvae_prof_row.kernel_ms were added after version 1; a client compiled against an older header passes shorter
 *    structs, so every binding checks dmvae_abi_version() == DMVAE_ABI_VERSION when it loads the library. */
/* 3: dmvae_plan_set_stage_groups added (no struct changed). */
/* 4: dmvae_plan_prefetch_batch / dmvae_plan_swap_batch added (a second bf16 batch buffer in the plan's workspace:
 *    dmvae_sizes.work_bytes grows; no struct layout changed). */
/* 5: dmvae_heads_latent_fwd / dmvae_heads_latent_ok / dmvae_heads_args added; DMVAE_ADAM_SHADOW flag of dmvae_adam_tf
 *    (no existing struct changed). */
#define DMVAE_ABI_VERSION 5

enum { DMVAE_F32 = 0, DMVAE_BF16 = 1 };

enum {
    DMVAE_EINVAL = -1,   /* bad argument (shape not tile aligned, null pointer ...) */
    DMVAE_EUNSUPPORTED = -2,
    DMVAE_ESTATE = -3
};

/* ---- operand layouts of dmvae_gemm -------------------------------------
 * C[M,N] = sum_k A(m,k) * B(k,n)
 *   DMVAE_GEMM_FWD : A = act [M][lda] (k contiguous),  B = W [K][ldb] (n contiguous)
 *                    tf.layers.dense / tf.matmul forward   base_models.py:221-248,291-293, includes/layers.py:32
 *   DMVAE_GEMM_DX  : A = dY  [M][lda] (k contiguous),  B = W [N][ldb] (k contiguous)
 *                    dX = dY . W^T  (tf.gradients of the above, base_models.py:110)
 *   DMVAE_GEMM_DW  : A = X   [K][lda] (m contiguous),  B = dY [K][ldb] (n contiguous)
 *                    dW = X^T . dY  (tf.gradients of the above)
 * M, N must be multiples of 64 and K of 64 (callers pad; see dmvae_plan).
 */
enum { DMVAE_GEMM_FWD = 0, DMVAE_GEMM_DX = 1, DMVAE_GEMM_DW = 2 };

/* ---- fused epilogues ---------------------------------------------------- */
enum {
    DMVAE_EPI_BIAS_RELU = 0, /* out(act) = relu(acc + bias[n])                    activation=relu dense      */
    DMVAE_EPI_BIAS_F32 = 1,  /* out(f32) = acc + bias[n]                          linear heads               */
    DMVAE_EPI_BIAS_RECON = 2,/* l = acc + bias; loss partial + out(act) = dLoss/dl  base_models.py:72-85       */
    DMVAE_EPI_RELU_MASK = 3, /* out(act) = acc * (aux0(act)[m][n] > 0)            ReLU backward              */
    DMVAE_EPI_LATENT = 4,    /* dZ = acc: out[m][n] = dZ + aux0, out[m][d_off+n] = dZ*aux2 + aux1   priors.py:86-89 backward */
    DMVAE_EPI_STORE_F32 = 5, /* out(f32) = acc            (dW, split_k == 1)                                    */
    DMVAE_EPI_ATOMIC_F32 = 6,/* out(f32) += acc via atomics (dW, split_k > 1; out pre-zeroed)                   */
    DMVAE_EPI_BIAS_SIGMOID = 7,/* out(f32) = sigmoid(acc + bias)  reconstructed_X  base_models.py:295-296      */
    DMVAE_EPI_ADAM = 8       /* dW only, grouped bf16 launch with a dmvae_adam_ctx: the gradient tile never
                              * leaves the registers -- the TF-Adam update of the matching parameter / m / v
                              * elements (same offset in every arena) is applied in the epilogue; out = the
                              * tile's address in the GRADIENT arena (locates the offset; written only when
                              * ctx->store_grad), out2 = the bias gradient's address there (updated likewise) */
};

typedef struct dmvae_epilogue {
    int32_t kind;        /* DMVAE_EPI_*                                              */
    int32_t m_valid;     /* rows  < m_valid are real (RECON masks the rest), 0 = all */
    int32_t n_valid;     /* cols  < n_valid are real (RECON masks the rest), 0 = all */
    int32_t d_off;       /* LATENT: column offset of the log_var half                */
    int32_t recon_kind;  /* RECON: 0 = binary (sigmoid xent), 1 = real (0.5*sq err)  */
    float scale;         /* RECON: 1/B                                               */
    void* out;           /* primary output                                           */
    int64_t ldo;
    void* out2;          /* RECON: optional f32 copy of the logits (may be NULL).
                          * DW layout: optional f32 bias gradient db[N] = sum_k B[k][n]
                          * (ones-operand MFMA in the first tile row; may be NULL)    */
    int64_t ldo2;
    const float* bias;   /* [N] or NULL                                              */
    const void* aux0;    /* RELU_MASK: forward activation (act); RECON: x (f32); LATENT: gmu (f32) */
    int64_t ld0;
    const void* aux1;    /* LATENT: glv (f32) */
    int64_t ld1;
    const void* aux2;    /* LATENT: clv = eps*0.5*exp(lv/2) (f32) */
    int64_t ld2;
    float* partials;     /* RECON: per-workgroup loss partial sums, length >= dmvae_gemm_partials() */
} dmvae_epilogue;

/* GEMM with fused epilogue.  dtype selects bf16 MFMA (v_mfma_f32_16x16x32_bf16,
 * fp32 accumulate) or exact-f32 MFMA (v_mfma_f32_16x16x4_f32).  split_k > 1 is
 * valid only with DMVAE_EPI_ATOMIC_F32. */
int dmvae_gemm(void* stream, int dtype, int layout, int M, int N, int K,
               const void* A, int64_t lda, const void* B, int64_t ldb,
               const dmvae_epilogue* epi, int split_k);
/* number of loss partials dmvae_gemm writes for an (M,N) RECON launch: one per 64x64 cell of the output,
 * whatever tile the kernel uses (a larger tile writes its sum to its first cell and zeros to the others) */
int dmvae_gemm_partials(int dtype, int M, int N);

/* Grouped weight-gradient GEMMs: n (<= 16) independent DMVAE_GEMM_DW problems
 * (dW_l = X_l^T . dY_l, optional fused db_l through epi.out2; epi.kind must be
 * DMVAE_EPI_STORE_F32) enqueued as ONE grid for bf16 -- every tf.gradients(loss, W_l)
 * of base_models.py:110 in one launch.  Each problem alone covers a fraction of the
 * 256 CUs; together they keep the chip full without split-K (bit-reproducible). */
typedef struct dmvae_gemm_problem {
    int32_t M, N, K, reserved;
    const void* A; int64_t lda;
    const void* B; int64_t ldb;
    dmvae_epilogue epi;
} dmvae_gemm_problem;
int dmvae_gemm_grouped_dw(void* stream, int dtype, const dmvae_gemm_problem* probs, int n);
/* the general form: n independent problems of one layout sharing an epilogue kind.  bf16 groups
 * exist for (DW, STORE_F32), (FWD, BIAS_F32) and (DX, RELU_MASK); f32 issues one launch each. */
int dmvae_gemm_grouped(void* stream, int dtype, int layout, const dmvae_gemm_problem* probs, int n);

/* dW GEMMs with the optimizer step fused into their epilogue (DMVAE_EPI_ADAM; bf16): replaces the
 * tf.gradients + AdamOptimizer.apply_gradients pair of base_models.py:95-110 for every weight and
 * bias in one launch.  The four arenas (param, grad, m, v) share one layout; t = state->adam_t
 * (already advanced for this step).  [seg_off, seg_off + seg_n) is an extra element range of the
 * arenas (multiple of 4 elements) whose gradient is already in `grad` -- the prior tables -- updated
 * by one more workgroup of the same launch. */
typedef struct dmvae_adam_ctx {
    float* param; float* grad; float* m; float* v;
    void* param_bf16;          /* bf16 shadow refreshed with the new parameters (may be NULL) */
    const void* state;         /* dmvae_state: lr and adam_t                                  */
    float beta1, beta2, epsilon, grad_scale;
    int32_t store_grad;        /* also write the gradients to `grad`                          */
    int32_t ieee;              /* bf16 mode: 1 = IEEE square root and division in the update quotient (as fp32 mode),
                                * 0 = the hardware v_sqrt_f32 / v_rcp_f32 (1 ulp each; dmvae_adam_tf below)      */
    int64_t seg_off, seg_n;
} dmvae_adam_ctx;
int dmvae_gemm_grouped_dw_adam(void* stream, const dmvae_gemm_problem* probs, int n, const dmvae_adam_ctx* ctx);

/* ---- latent kernel: softmax + reparameterisation + mixture KL + all KL gradients
 * replaces priors.py:86-89 (Z), :104-147 (KL_Z exact / relaxed), :170-181
 * (Gumbel-Softmax), :183-201 (KL_C), base_models.py:249 (softmax) and their
 * tf.gradients.  mode 0 = exact (cluster_sample False, live), 1 = relaxed, 2 = VaDE (below). */
typedef struct dmvae_latent_args {
    int32_t B;            /* rows that are real; rows [B, B_pad) are written as zeros */
    int32_t B_pad;
    int32_t D, K;
    int32_t mode;         /* 0 exact, 1 relaxed (Gumbel-Softmax weights)              */
    int32_t act_dtype;    /* dtype of Z_act / dlogits_act                              */
    float kl_ratio;       /* used when state == NULL                                  */
    float temperature;
    float inv_B;          /* 1 / (batch size the loss averages over)                  */
    uint64_t seed;        /* Philox key when eps / gumbel are NULL                    */
    uint64_t noise_step;  /* Philox stream position when state == NULL                */
    const float* mean; int64_t ld_mean;       /* [B_pad][>=D] */
    const float* log_var; int64_t ld_log_var; /* [B_pad][>=D] */
    const float* logits; int64_t ld_logits;   /* [B_pad][>=K] */
    const float* eps; int64_t ld_eps;         /* [B][D] or NULL -> on-device Philox N(0,1)   */
    const float* gumbel; int64_t ld_gumbel;   /* [B][K] or NULL -> on-device Philox Gumbel    */
    const float* prior_means;                 /* [K][D] */
    const float* prior_log_vars;              /* [K][D] */
    void* Z_act; int64_t ld_Z;                /* [B_pad][ld_Z] act dtype; cols >= D zeroed    */
    float* Z_f32; int64_t ld_Zf;              /* optional f32 copy or NULL                    */
    float* weights; int64_t ld_w;             /* optional [B_pad][K]: softmax(logits) / zeta  */
    float* gmu; float* glv; float* clv; int64_t ld_g;  /* [B_pad][ld_g] f32: KL grads wrt mean/log_var, reparam coef */
    void* dlogits_act; int64_t ld_dl;         /* [B_pad][ld_dl] act dtype; cols >= K zeroed   */
    float* dprior_partials;                   /* [nblocks][2][K][D] f32 (deterministic two-pass) */
    float* loss_partials;                     /* [nblocks][2]: sum_b KL_Z_b, sum_b KL_C_b      */
    const void* state;                        /* optional dmvae_state* (device): kl_ratio, noise_step read from it */
    /* Large prior tables (mode 0, K * D >= 4096: dmvae_latent_ws_bytes() > 0): scratch for the MFMA form of the
     * (row, cluster, dimension) contractions -- three exact-f32 MFMA GEMMs between two row-wise kernels
     * (csrc/latent_mfma.hip).  NULL (or too small a size) = the one-kernel form.  With the scratch, the loss partials
     * are written for the same dmvae_latent_nblocks() blocks, but the prior-table gradient arrives COMPLETE in row 0
     * of dprior_partials (rows 1.. are not touched), and on-device noise comes from a differently keyed Philox stream. */
    void* mfma_ws; int64_t mfma_ws_bytes;
} dmvae_latent_args;
int dmvae_latent_nblocks(int B_pad, int D, int K);
/* mode 2 (VaDE, csrc/latent_vade.hip): weights = get_cluster_probs(Z) of the SAMPLE (priors.py:91-102) for both KL terms,
 * gradients through them included; logits / gumbel / dlogits_act are ignored (may be NULL); `weights` receives the
 * responsibilities.  It writes dmvae_latent_nblocks_vade(B_pad) = B_pad / 16 blocks of partials. */
int dmvae_latent_nblocks_vade(int B_pad);
/* Prior tables past the LDS of that kernel -- 4 (2 K (D + 1) + 33 K + 64 (D + 1) + 32) bytes > 60 KiB: D = 256 at any K, D = 128 from
 * K = 11 on -- take the large-table form (csrc/latent_vade_mfma.hip: the contractions as exact-f32 MFMA GEMMs between row kernels),
 * for any D and K (mode 2 is dispatched before, and shares none of, the LDS limit of modes 0 and 1; what bounds it is the memory for
 * its scratch).  It needs scratch in mfma_ws / mfma_ws_bytes (without it: DMVAE_EINVAL), linear in B D + B K + K D:
 * dmvae_latent_vade_ws_bytes, pure host arithmetic, returns its size -- 0 where the one-kernel form runs (forced = 0), or what the
 * large-table form would need at any shape (forced = 1: debug knob 22); *n_slabs (may be NULL): the batch slabs of its two
 * prior-table contractions together.  Loss partials as above; the prior-table gradient arrives COMPLETE in row 0 of
 * dprior_partials.  Device noise of this form: the keying of csrc/latent_mfma.hip.  dmvae_latent_ws_bytes(.., mode 2) is
 * dmvae_latent_vade_ws_bytes(.., 0, NULL). */
int64_t dmvae_latent_vade_ws_bytes(int B_pad, int D, int K, int forced, int* n_slabs);
int64_t dmvae_latent_ws_bytes(int B_pad, int D, int K, int mode);   /* 0 when the MFMA form does not apply */
int dmvae_latent_fwd(void* stream, const dmvae_latent_args* a);

/* ---- the two head layers' forward pass AND the latent stage as one launch (csrc/heads_latent.hip) -----------------
 * [mean | log_var] = hz . W_mv + b_mv and logits = hc . W_lg + b_lg (the three linear tf.layers.dense of base_models.py:229-249:
 * 231-239 mean / log_var off the z-head's hidden layer, 241-248 logits off the c-head's) followed, on the same rows in the same
 * workgroup, by everything dmvae_latent_fwd computes (priors.py:86-201).  `a` as for dmvae_latent_fwd, except that a->mean,
 * a->log_var (= a->mean + Dp, one [B_pad][2 Dp] buffer) and a->logits ([B_pad][Kp]) are OUTPUTS here: the heads' f32 results are
 * written there as dmvae_gemm with DMVAE_EPI_BIAS_F32 would write them -- same bits -- and every other output is bit-identical to
 * dmvae_gemm_grouped + dmvae_latent_fwd on the same inputs.  bf16 operands only; Dp = 64 | 128, Kp = 64, K * D < 4096 (the one-kernel
 * latent form), Hp a multiple of 64, B_pad a multiple of 16 and at most 4096 (one round of 256 workgroups: every workgroup streams
 * both weight matrices); anything else: DMVAE_EUNSUPPORTED (dmvae_heads_latent_ok() == 0) -- use the two calls. */
typedef struct dmvae_heads_args {
    const void* hz; int64_t lda;     /* bf16 [B_pad][lda]: columns [0, Hp) = relu hidden layer of the z-head, [Hp, 2 Hp) = of the c-head */
    int32_t Hp, Dp, Kp, reserved;    /* padded widths: head hidden layer, latent_dim, n_classes                                       */
    const void* W_mv; int64_t ld_mv; /* bf16 [Hp][ld_mv]: columns [0, Dp) mean's kernel, [Dp, 2 Dp) log_var's                         */
    const void* W_lg; int64_t ld_lg; /* bf16 [Hp][ld_lg]: the logits kernel                                                           */
    const float* b_mv;               /* f32 [2 Dp] */
    const float* b_lg;               /* f32 [Kp]   */
    /* K slices (optional; small batches: few 16-row blocks, each a long K chain): kslices (2 .. 8, Hp % (kslices * 64) == 0) workgroups per block,
     * whose partial tiles the last one to arrive adds in ascending order before the latent stage -- deterministic; the results then differ from the
     * unsliced call by the f32 summation order.  kslice_ws: >= dmvae_heads_latent_kslice_floats() floats; kslice_tick: B_pad / 16 ints, zero on
     * entry (left zero).  kslices <= 1: none. */
    int32_t kslices, reserved2;
    float* kslice_ws; int64_t kslice_ws_floats;
    int32_t* kslice_tick;
} dmvae_heads_args;
int64_t dmvae_heads_latent_kslice_floats(int B_pad, int Dp, int kslices);
int dmvae_heads_latent_ok(int B_pad, int D, int K, int Dp, int Kp, int Hp, int mode);
int dmvae_heads_latent_fwd(void* stream, const dmvae_heads_args* heads, const dmvae_latent_args* a);

/* ---- stand-alone reconstruction loss (fused form: DMVAE_EPI_BIAS_RECON) --
 * tf.nn.sigmoid_cross_entropy_with_logits + reduce_sum/mean, base_models.py:72-85 */
int dmvae_recon_fwd_bwd(void* stream, int act_dtype, int recon_kind, int B, int B_pad, int I, int I_pad,
                        const float* logits, int64_t ldl, const float* x, int64_t ldx, float inv_B,
                        void* dlogits_act, int64_t ldd, float* partials /* [dmvae_recon_nblocks] */);
int dmvae_recon_nblocks(int B_pad, int I_pad);

/* ---- column sums (bias gradients, reduction of per-block partials) ------
 * out[n] = sum_m in[m][n]; tf.gradients of the bias add. */
int dmvae_colsum(void* stream, int in_dtype, const void* in, int64_t ld, int M, int N, float* out);

/* ---- device-resident step state (read by kernels so a captured graph can be replayed) */
typedef struct dmvae_state {
    uint64_t adam_t;        /* completed Adam updates (t of the next update = adam_t + 1) */
    uint64_t noise_step;    /* Philox stream position                                  */
    uint32_t batch_cursor;  /* next batch within the epoch                             */
    uint32_t batches_per_epoch;
    float kl_ratio;
    float lr;
    float epoch_weight;     /* 1/epoch_len: loss += batch_loss * epoch_weight  (base_models.py:130) */
    float lr_t;             /* lr*sqrt(1-b2^t)/(1-b1^t) for t = adam_t, written when a plan step advances adam_t
                             * (read by the fused dW + Adam epilogue; the stand-alone Adam kernel recomputes it) */
    float epoch_loss, epoch_recon, epoch_klz, epoch_klc;   /* running epoch means   */
    float last_loss, last_recon, last_klz, last_klc;       /* last batch            */
} dmvae_state;

/* loss = recon + kl_ratio*(KL_C + KL_Z)  (base_models.py:87-93); sums the
 * per-block partials deterministically, updates state (epoch accumulators,
 * batch_cursor, noise_step). */
int dmvae_loss_finalize(void* stream, const float* recon_partials, int n_recon,
                        const float* latent_partials, int n_latent, float inv_B, void* state);

/* ---- TF-1.x Adam on a flat arena (tf.train.AdamOptimizer, base_models.py:95-110)
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t); theta -= lr_t*m/(sqrt(v)+eps).  t = state->adam_t+1
 * (or t_host when state is NULL).  grad is multiplied by grad_scale first (1/world).
 * Optionally refreshes a bf16 shadow of the parameters and zeroes grad (flags & DMVAE_ADAM_ZERO_GRAD).
 * Arithmetic follows the mode: param_bf16 == NULL (fp32 parity mode) -> IEEE sqrt and division; param_bf16 != NULL (bf16
 * throughput mode, where the forward pass reads the 8-bit-mantissa shadow) -> the quotient lr_t*m / (sqrt(v)+eps) with
 * the hardware square root and reciprocal (1 ulp each), exactly as the fused dW + Adam epilogues of that mode compute it
 * (DMVAE_EPI_ADAM: bit-identical to this kernel on the same inputs); flags & DMVAE_ADAM_IEEE keeps IEEE there too.
 * dmvae_adam_finish bumps state->adam_t (separate 1-thread kernel so that all
 * chunks of one update see the same t). */
#define DMVAE_ADAM_ZERO_GRAD 1
#define DMVAE_ADAM_IEEE 2
/* the same update (same bits) on the low-footprint kernel that can share a CU with a macro-tile GEMM running on another stream
 * (<= 48 VGPRs, a 32 KiB LDS ring filled by LDS-DMA, four waves per workgroup); bits 8..23 of flags: workgroups (0 = 256) */
#define DMVAE_ADAM_SHADOW 4
int dmvae_adam_tf(void* stream, int64_t n, float* param, float* grad, float* m, float* v,
                  void* param_bf16, float lr, float beta1, float beta2, float epsilon,
                  float grad_scale, int flags, uint64_t t_host, const void* state);
int dmvae_adam_finish(void* stream, void* state);

/* ---- batch assembly (Dataset.get_batches, includes/utils.py:449-463) -----
 * row r of the batch = data[perm[first + r]] (perm NULL: data[first + r]);
 * first = cursor*batch (cursor from state when state != NULL).  Writes the act
 * copy [B_pad][ld_act] and an f32 copy (either may be NULL); pad rows/cols = 0. */
int dmvae_gather_rows(void* stream, int act_dtype, const float* data, int64_t n_rows, int dim,
                      const int32_t* perm, int64_t first, int batch, int n_valid, int B_pad,
                      void* out_act, int64_t ld_act, float* out_f32, int64_t ld_f32,
                      const void* state);

/* ---- noise (np.random.randn / sample_gumbel, priors.py:67-68,157-158) ---- */
int dmvae_philox_normal(void* stream, float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t stream_id);
int dmvae_philox_gumbel(void* stream, float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t stream_id);
/* uniform in [0, 1): (x >> 8) * 2^-24 of the stream's 32-bit words, word i & 3 of Philox block i >> 2 (the draws of dmvae_gmm_seed) */
int dmvae_philox_uniform(void* stream, float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t stream_id);

/* ---- casts ---- */
int dmvae_cast_f32_to_bf16(void* stream, const float* in, void* out, int64_t n);
int dmvae_cast_bf16_to_f32(void* stream, const void* in, float* out, int64_t n);

/* ======================================================================
 * Step plan: the whole session.run([loss, train_step]) as one enqueue.
 * ====================================================================== */
#define DMVAE_MAX_LAYERS 8
/* Encoder trunk.  MLP: tf.layers.dense x n_enc on the 784 inputs (base_models.py:218-226, the branch
 * BASELINE.json names).  CNN: the checked-in `self.cnn = True` branch (base_models.py:156,176-216): the
 * batch as 28x28x1 images, six 3x3 SAME convolutions (32,32,64,64,128,128) with 2x2 SAME max-pools behind
 * the 2nd / 4th / 6th, flattened (h,w,c) to 2048, then ONE FullyConnected layer enc[0] (n_enc must be 1,
 * input_dim 784).  The conv layers run as the step's GEMMs in conv mode -- the patch matrix is implicit,
 * activations are stored with a zero border (csrc/conv.hip).  Their tensors come first in the arena:
 * "W_conv<i>" [9*Cin][Cout] = the HWIO kernel flattened (ld = Cout padded to 64) and "b_conv<i>" [Cout]. */
#define DMVAE_TRUNK_MLP 0
#define DMVAE_TRUNK_CNN 1
/* Model.  DMVAE: base_models.py:150-302 (trunk, z-head and c-head with a hidden layer each, q(c|x) = softmax(logits)).
 * VaDE: base_models.py:435-562 -- n_enc FullyConnected trunk layers, mean / log_var linear straight off the trunk (no
 * head hidden layers, no logits: head_dim is ignored), q(c|x) := p(c|z) = get_cluster_probs(Z) (priors.py:91-102) as the
 * mixture weights AND the categorical probabilities; the latent stage is dmvae_latent_fwd mode 2.  Tensor table: W_enc<i>,
 * b_enc<i>, W_mean, b_mean, W_logvar, b_logvar, W_dec<i>, b_dec<i>, W_out, b_out, prior_means, prior_log_vars.
 * With DMVAE_TRUNK_CNN (base_models.py:456-488): the same conv / pool stack in front, enc[0] = 128 (fc 2048 -> 128). */
#define DMVAE_MODEL_DMVAE 0
#define DMVAE_MODEL_VADE 1

typedef struct dmvae_config {
    int32_t input_dim, latent_dim, n_classes;
    int32_t n_enc; int32_t enc[DMVAE_MAX_LAYERS];   /* trunk widths (reference: 500,500)        */
    int32_t head_dim;                                /* z-/c-head hidden width (reference: 2000) */
    int32_t n_dec; int32_t dec[DMVAE_MAX_LAYERS];   /* decoder widths (reference: 2000,500,500) */
    int32_t input_type;                              /* 0 binary, 1 real                         */
    int32_t dtype;                                   /* DMVAE_F32 (parity) or DMVAE_BF16         */
    int32_t max_batch;                               /* largest per-rank batch                   */
    int32_t mode;                                    /* 0 exact KL, 1 relaxed (Gumbel-Softmax)   */
    float temperature;
    float beta1, beta2, adam_eps;
    uint64_t seed;
    int32_t deterministic;                           /* 1: no float atomics anywhere             */
    int32_t trunk;                                   /* DMVAE_TRUNK_MLP (default) or DMVAE_TRUNK_CNN */
    int32_t model;                                   /* DMVAE_MODEL_DMVAE (default) or DMVAE_MODEL_VADE */
    int32_t adam_ieee;                               /* bf16 plans: 1 = TF-Adam with the IEEE square root and division (exactly the
                                                      * fp32 mode's arithmetic on the fp32 master weights); 0 (default) = hardware
                                                      * sqrt / reciprocal, 1 ulp each (-0.06 ms at cfg5)                */
} dmvae_config;

typedef struct dmvae_tensor_info {
    char name[32];
    int64_t offset;      /* element offset in the parameter arena */
    int32_t rows, cols;  /* logical shape (rows = 1 for biases)   */
    int64_t ld;          /* row stride in elements                */
} dmvae_tensor_info;

typedef struct dmvae_sizes {
    int64_t param_elems;     /* f32 arena (also grad, m, v; and the bf16 shadow in elements) */
    int64_t work_bytes;      /* activation / scratch workspace                               */
    int32_t batch_pad;       /* padded batch rows                                            */
    int32_t input_pad;       /* padded input columns                                         */
    int32_t n_tensors;
    int32_t reserved;
} dmvae_sizes;

typedef struct dmvae_buffers {
    float* param; float* grad; float* m; float* v;
    void* param_bf16;     /* bf16 shadow (may be NULL when dtype == DMVAE_F32) */
    void* work;           /* work_bytes, 256-byte aligned, zero-initialised by the caller */
    void* state;          /* dmvae_state on the device */
    int64_t arena_elems;  /* elements allocated for each of param / grad / m / v (/ shadow): >= param_elems; a caller that
                           * cuts the arenas into equal slices per rank (reduce-scatter -> sharded Adam -> all-gather) pads
                           * them, and dmvae_plan_update_range then accepts ranges up to this size.  0 = param_elems */
} dmvae_buffers;

typedef struct dmvae_plan dmvae_plan;

int dmvae_plan_create(const dmvae_config* cfg, dmvae_plan** out);
void dmvae_plan_destroy(dmvae_plan* p);
int dmvae_plan_sizes(const dmvae_plan* p, dmvae_sizes* out);
int dmvae_plan_tensor(const dmvae_plan* p, int index, dmvae_tensor_info* out);
int dmvae_plan_bind(dmvae_plan* p, const dmvae_buffers* b);

/* batch assembly into the plan's input buffers (see dmvae_gather_rows) */
int dmvae_plan_load_batch(dmvae_plan* p, void* stream, const float* data, int64_t n_rows,
                          const int32_t* perm, int64_t first, int n_valid, int use_state_cursor);
/* The same for a caller that goes straight on to ONE dmvae_plan_forward_backward / _train_step on this batch.  On bf16 plans whose
 * output layer the small-tile kernel runs (input_dim a multiple of 4) only the bf16 copy of the batch is written: the f32 copy's one
 * reader in a step, the reconstruction epilogue of the output layer (base_models.py:72-85), fetches its target rows from `data`
 * through `perm` itself.  `data` and `perm` must stay alive and unchanged until that step has run; the "x" view is not valid
 * afterwards.  Any other plan: exactly dmvae_plan_load_batch. */
int dmvae_plan_load_batch_step(dmvae_plan* plan, void* stream, const float* data, int64_t n_rows, const int32_t* perm,
                               int64_t first, int n_valid, int use_state_cursor);
/* Batch assembly overlapped with the step (Dataset.get_batches, includes/utils.py:449-463, one batch ahead): arms the assembly of the NEXT
 * batch inside the next dmvae_plan_forward_backward / _train_step -- by workgroups riding in one of its launches where that launch leaves
 * them room, else by a gather launch of its own -- into the other of the plan's two bf16 batch buffers; with use_state_cursor the rows are
 * those of the device cursor after that pass has advanced it.  dmvae_plan_swap_batch (host state only) then makes that batch the current
 * one, in place of the dmvae_plan_load_batch_step in front of the following step.  DMVAE_EUNSUPPORTED on plans that assemble their batches
 * with dmvae_plan_load_batch (f32, conv trunk, output layer on the macro tile).  `data` / `perm`: alive and unchanged until the step that
 * CONSUMES the prefetched batch has run -- i.e. the step AFTER the one that assembles it (its reconstruction epilogue reads the targets
 * through them).  A captured step holds the buffer it was captured with: capture one graph per buffer and alternate them. */
int dmvae_plan_prefetch_batch(dmvae_plan* plan, const float* data, int64_t n_rows, const int32_t* perm, int64_t first, int n_valid,
                              int use_state_cursor);
int dmvae_plan_swap_batch(dmvae_plan* plan);
/* forward + loss + backward: fills the grad arena and the loss partials.
 * eps / gumbel: caller-supplied noise (parity mode) or NULL (on-device Philox). */
int dmvae_plan_forward_backward(dmvae_plan* p, void* stream, int n_valid,
                                const float* eps, int64_t ld_eps, const float* gumbel, int64_t ld_gumbel,
                                float inv_B);
/* The same work cut into three segments for data parallelism: after segment k one contiguous
 * bucket of the gradient arena is final, so its all-reduce can run while the next segment computes
 * (the reference has no counterpart: it is single-process).  Segment 0 = forward, loss, decoder
 * backward; 1 = heads backward; 2 = trunk backward; call them in order with the same arguments.
 * dmvae_plan_grad_buckets: bounds[5] in arena elements.  The arena holds every weight matrix first and, from
 * bounds[3] (a multiple of 4096) on, the small fp32 tensors: every bias, then the prior tables.  Segment 0 completes
 * the weights [bounds[2], bounds[3]), segment 1 [bounds[1], bounds[2]), segment 2 [bounds[0], bounds[1]); the tail
 * [bounds[3], bounds[4]) is complete when segment 2 has run.  A data-parallel caller can reduce-scatter the weight
 * buckets, update its owned slices and all-gather the bf16 SHADOW of the weights (the GEMMs read nothing else of
 * them), and all-reduce + update the tail on every rank (the epilogues and the latent kernel read it in fp32).
 * Results are bit-identical to dmvae_plan_forward_backward. */
int dmvae_plan_forward_backward_stage(dmvae_plan* p, void* stream, int stage, int n_valid,
                                      const float* eps, int64_t ld_eps, const float* gumbel, int64_t ld_gumbel,
                                      float inv_B);
int dmvae_plan_grad_buckets(const dmvae_plan* p, int64_t bounds[5]);
/* How many weight-gradient launches the staged backward issues: 3 (default) = one per segment, as above; 2 = segment 0's
 * weight-gradient problems stay queued and go out with segment 1's in ONE grouped launch, so that [bounds[1], bounds[3])
 * -- decoder + heads, 86 % of the weights of the MNIST-shaped stacks -- is complete when segment 1 has run and its
 * collective can overlap segment 2 (the trunk), at the price of two weight-gradient grids per step instead of three
 * (MNIST-sized arenas: three small grids fill the chip worse than they hide wire time).
 * Results stay bit-identical to dmvae_plan_forward_backward. */
int dmvae_plan_set_stage_groups(dmvae_plan* p, int n_groups);
/* Adam (+ bf16 shadow refresh); grad_scale = 1/world_size.  The loss finalize at the end of
 * dmvae_plan_forward_backward has already advanced state->adam_t for this step: every
 * forward_backward is to be followed by exactly one update. */
int dmvae_plan_update(dmvae_plan* p, void* stream, float grad_scale);
/* the same on the arena elements [lo, hi) only (4-aligned): with the bucketed gradient exchange each
 * bucket is updated as soon as its all-reduce has landed, while later buckets are still in flight */
int dmvae_plan_update_range(dmvae_plan* p, void* stream, float grad_scale, int64_t lo, int64_t hi);
/* forward + loss + backward + Adam as ONE sequence with the update fused into the dW launch
 * (single-process training on a bf16 plan: no gradient exchange between backward and update).
 * Equivalent to dmvae_plan_forward_backward followed by dmvae_plan_update(grad_scale = 1), except
 * that the gradient arena is not written.  f32 plans run exactly that pair. */
int dmvae_plan_train_step(dmvae_plan* p, void* stream, int n_valid,
                          const float* eps, int64_t ld_eps, const float* gumbel, int64_t ld_gumbel,
                          float inv_B);
/* inference pieces used by get_accuracy / reconstruction / sampling:
 * encode: X (loaded batch) -> mean, log_var, logits (f32, in the workspace)
 * decode: Z (f32 [n][latent_dim], caller) -> sigmoid/identity reconstruction (f32, workspace) */
int dmvae_plan_encode(dmvae_plan* p, void* stream, int n_valid);
int dmvae_plan_decode(dmvae_plan* p, void* stream, const float* Z, int64_t ldz, int n_valid);
/* workspace views: name in {"mean","log_var","logits","recon","weights","Z","xlogits","x"} and, on VaDE plans, "eval_w"
 * (dmvae_plan_eval_clusters);
 * returns the device pointer, leading dimension (elements) and dtype. */
int dmvae_plan_view(const dmvae_plan* p, const char* name, void** ptr, int64_t* ld, int32_t* dtype);

/* ---- mixture-of-experts head on the gate (models.py:10-163 of the reference: DeepMoE = dmoe, DeepVariationalMoE = dvmoe) -----
 * Attached to a DMVAE plan (MLP trunk, one rank) between dmvae_plan_create and dmvae_plan_sizes / bind.  The gate is the step's
 * q = softmax(logits) (base_models.py:249, both KL modes), E = n_experts = the plan's n_classes.  Expert input: the batch X (featLearn 0)
 * or relu(mean) (featLearn 1).  Tensors: "W_moe" [in][E*O] (column e*O + o; the reference's regression_weights[e][o][i] = W_moe[i][e*O+o])
 * is the LAST weight matrix of the arena and "b_moe" [E*O] (regression_biases[o][e]) the last bias before the prior tables.
 * Every step of the plan then adds the MoE loss (classification: models.py:83-105,141-144; regression: :106-113,145-146) and its
 * gradients (scaled by inv_B, not by kl_ratio); lossVAE 0 (dmoe) scales the VAE terms' gradients by zero (loss = loss_moe).
 * Labels: [label_rows][O] f32 on the device, read through the batch permutation of the last batch load (device cursor included),
 * so a captured step needs no host argument.  Accumulators: the "moe_acc" view, 4 floats: [0] += loss_moe of every batch,
 * [1] += its error (classification: wrong rows; regression: mean squared error * O), [2] / [3] = the last batch's; the caller
 * zeroes them.  Limits: E <= 256, O <= 64, E * O <= 1024 (DMVAE_EINVAL); conv trunk, VaDE, staged backward, prefetched batches and
 * plans with dW K-slices (>= 8192 rows): DMVAE_EUNSUPPORTED. */
typedef struct dmvae_moe_config {
    int32_t n_experts;       /* E: must equal the plan's n_classes      */
    int32_t output_dim;      /* O                                        */
    int32_t featLearn;       /* 0: experts read X; 1: relu(mean)         */
    int32_t classification;  /* 1: softmax experts; 0: regression        */
    int32_t lossVAE;         /* 1: loss = loss_moe + vae.loss; 0: loss_moe only */
    int32_t reserved;
    const float* labels;     /* device [label_rows][O] f32               */
    int64_t label_rows;
} dmvae_moe_config;
int dmvae_plan_attach_moe(dmvae_plan* p, const dmvae_moe_config* cfg);
/* another label array (e.g. the test set's) for the following steps / predictions (host state only; a captured step keeps its own) */
int dmvae_plan_moe_set_labels(dmvae_plan* p, const float* labels, int64_t label_rows);
/* forward only (get_accuracy / predict): encode the loaded batch, experts, gate, mixture; writes the "moe_pred" view [B_pad][O]
 * (reconstructed_Y_soft / reconstructed_Y) and adds loss and error to the accumulators; no gradient, no state change */
int dmvae_plan_moe_predict(dmvae_plan* p, void* stream, int n_valid);

/* ---- semi-supervised DMVAE: cross-entropy on q(c|x) = softmax(logits) for the batch rows that carry a label (label_xent.hip) ----
 * Batch row r < n_valid is data-set row i_r = perm[first + r] (perm NULL: first + r); its label y_r = labels[i_r], labels a device
 * int32 [label_rows] array in data-set row order, -1 = no label.  For the labelled rows
 *     l_r = logsumexp(logits_r[0..K)) - logits_r[y_r]               (f32, the maximum subtracted)
 *     dlogits_r[k] += coefficient * (softmax(logits_r)[k] - [k == y_r])      (act dtype: f32 add, then round to nearest even)
 * and NOTHING else of dlogits is written: rows without a label, rows >= n_valid, columns >= K keep their bits, and every row does while
 * the coefficient is zero.  A label outside {-1} u [0, K) sets bit 0 of *err_flag, a row index outside [0, label_rows) bit 1 (device
 * int32, the caller zeroes it); such a row is skipped and nothing is read out of bounds (the rule of dmvae_plan_eval_clusters).
 *
 * dmvae_label_xent: the stage alone on caller buffers; the launcher the plan calls.  coefficient = scale.  row_loss (may be NULL):
 *   f32 [n_valid], l_r, 0 in rows without a label.  acc: device float64 [dmvae_label_xent_acc_elems(n_valid)], zeroed ONCE by the caller:
 *   [0] += sum of l_r (unweighted), [1] += labelled rows, [2] += rows whose arg-max (np.argmax's rule on ties: the first index of the
 *   largest, as dmvae_argmax_labels) equals the label; [3..6) = the same three of this launch alone; [6..8) and the rest are the launch's
 *   scratch (tickets, one partial triple per workgroup of four rows), which must be zero when a launch starts and which every launch
 *   leaves zero again: zero the buffer once, then only [0..6) as needed.  Counts are exact (< 2^53); the
 *   partials are added in workgroup order by the last workgroup to arrive: no float atomics, two runs give the same bits.  One launch
 *   (none when n_valid == 0); it only enqueues.  Every argument is checked by name before anything is enqueued (DMVAE_EINVAL): a null
 *   logits / labels / dlogits / acc / err_flag, K < 1, n_valid < 0, ld_lg < K, ld_dl < K, label_rows < 1, first < 0, without perm
 *   first + n_valid > label_rows, act_dtype not DMVAE_F32 / DMVAE_BF16, a scale that is not finite.
 *
 * dmvae_plan_attach_labels: between dmvae_plan_create and dmvae_plan_sizes / bind, like dmvae_plan_attach_moe.  Every pass of the plan
 *   then runs the stage behind its latent stage (one launch more; a plan without the attachment enqueues what it always did) on its own
 *   logits / dlogits with coefficient = w * inv_B (inv_B as passed to the pass, not scaled by kl_ratio), so the term reaches the c-head and
 *   the trunk and nothing else.  w is READ ON THE DEVICE from the "label_ctl" view (f32, [0] = w, written by the caller; 0 after the
 *   caller's zeroing of the workspace): a captured step follows a change of w without recapture.  Rows are addressed as the last batch load
 *   addressed them (device cursor included): a captured step needs no per-step host argument.  Views: "label_ctl"; "label_acc" (float64,
 *   the layout of acc above, ld = its element count; the caller zeroes it); "label_err" (int32, the error flag).  No new parameter, no
 *   new GEMM problem; the workspace grows only on attached plans.  Attaches to MLP and conv trunks, f32 and bf16, exact and relaxed KL
 *   mode, every batch size.  DMVAE_EUNSUPPORTED: VaDE plans (their q(c|x) is p(c|z): the gradient would run through Z into the VaDE
 *   latent stage) and plans with a MoE attachment (and dmvae_plan_attach_moe refuses a plan with labels).
 *   Staged backward (dmvae_plan_forward_backward_stage) is SERVED: the stage belongs to segment 0.  Prefetched batches
 *   (dmvae_plan_prefetch_batch) are SERVED too: the stage reads the cursor of the current batch, which step_finalize advances later in
 *   the same pass, and dmvae_plan_swap_batch hands the prefetched batch's rows on.
 * dmvae_plan_set_labels: another label array for the following passes (host state only; a captured step keeps its own). */
#define DMVAE_F64 2      /* dtype code of the "label_acc" view */
#define DMVAE_I32 3      /* dtype code of the "label_err" view */
typedef struct dmvae_label_config {
    const int32_t* labels;   /* device int32 [label_rows], -1 = no label */
    int64_t label_rows;
    int64_t reserved;        /* 0 */
} dmvae_label_config;
int64_t dmvae_label_xent_acc_elems(int n_valid);
int dmvae_label_xent(void* stream, const float* logits, int64_t ld_lg, int n_valid, int K, const int32_t* labels, int64_t label_rows,
                     const int32_t* perm, int64_t first, float scale, int act_dtype, void* dlogits, int64_t ld_dl, float* row_loss,
                     double* acc, int32_t* err_flag);
int dmvae_plan_attach_labels(dmvae_plan* p, const dmvae_label_config* cfg);
int dmvae_plan_set_labels(dmvae_plan* p, const int32_t* labels, int64_t label_rows);

/* ---- diagonal-covariance Gaussian mixture fit (the GMM initialisation of the prior tables, base_models.py:367-390, 614-646:
 * sklearn.mixture.GaussianMixture(covariance_type="diag")) ------------------------------------------------------------------
 * EM over X [N][ldx] f32 with n_init restarts side by side in one call; sklearn's semantics:
 *   E: lp_nk = log w_k - 1/2 [D log 2pi + sum_d log var_kd + sum_d (x_nd - mu_kd)^2 / var_kd], ll_n = logsumexp_k, resp = exp(lp - ll)
 *   M: nk = sum_n resp + 10 eps, w = nk / sum nk, mu = sum resp x / nk, var = sum resp x^2 / nk - mu^2 + reg_covar
 *   a restart stops once |lb - lb_prev| < tol (lb = mean_n ll) or after max_iter iterations; the restart with the largest final
 *   lower bound (the first on ties) is copied to the result.
 * Each restart starts from hard labels (labels [n_init][N], values in [0, K); the initial weights are weights_init when given) or from
 * centres (centers [n_init][K][D]): then Lloyd's k-means runs first (at most kmeans_iter iterations; it stops when no label changes or
 * sum_k ||c'_k - c_k||^2 <= 1e-4 * mean_d Var(X_d)) and its labels start the EM.  Exactly one of labels / centers is given.
 * No float atomics: per-workgroup partial statistics, added in block order, so two runs agree bit for bit.  The calls enqueue
 * 2 * (max_iter + kmeans_iter) + O(1) launches and never synchronise; a stopped restart's workgroups return at once.
 * Limits (tables and a 32-row tile live in LDS): K * D <= 3328, K <= 256 and 4 * (2 K (D + 1) + K + 32 (D + 1) + 32 (K + 1)) + 128 <= 65536
 * bytes, else DMVAE_EUNSUPPORTED. */
typedef struct dmvae_gmm_config {
    int32_t N, D, K;
    int32_t n_init;          /* restarts R >= 1                                    */
    int32_t max_iter;        /* EM iterations >= 1                                  */
    int32_t kmeans_iter;     /* Lloyd iterations (centers given / dmvae_gmm_kmeans) */
    float tol;               /* EM stopping threshold on the lower bound            */
    float reg_covar;
    int32_t flags;           /* reserved: 0                                         */
} dmvae_gmm_config;
/* device pointers of the caller; every one may be null except weights / means / covariances / lower_bound / n_iter / converged /
 * best_restart in dmvae_gmm_fit and centers / labels in dmvae_gmm_kmeans */
typedef struct dmvae_gmm_result {
    float* weights;          /* [K]     the selected restart                        */
    float* means;            /* [K][D]                                              */
    float* covariances;      /* [K][D]                                              */
    double* lower_bound;     /* [1]                                                 */
    int32_t* n_iter;         /* [1]                                                 */
    int32_t* converged;      /* [1]                                                 */
    int32_t* best_restart;   /* [1]                                                 */
    double* lower_bounds;    /* [n_init] per restart                                */
    int32_t* n_iters;        /* [n_init]                                            */
    int32_t* convergeds;     /* [n_init]                                            */
    float* all_weights;      /* [n_init][K]                                         */
    float* all_means;        /* [n_init][K][D]                                      */
    float* all_covariances;  /* [n_init][K][D]                                      */
    float* centers;          /* [n_init][K][D] Lloyd's final centres                */
    int32_t* labels;         /* [n_init][N]    and the labels of those centres      */
    int32_t* kmeans_iters;   /* [n_init]                                            */
} dmvae_gmm_result;
int64_t dmvae_gmm_ws_bytes(const dmvae_gmm_config* cfg);      /* < 0: an error code */
int dmvae_gmm_fit(void* stream, const dmvae_gmm_config* cfg, const float* X, int64_t ldx, const int32_t* labels, const float* centers,
                  const float* weights_init, void* ws, int64_t ws_bytes, dmvae_gmm_result* out);
/* Lloyd's k-means alone from centers [n_init][K][D]: out->centers, out->labels, out->kmeans_iters */
int dmvae_gmm_kmeans(void* stream, const dmvae_gmm_config* cfg, const float* X, int64_t ldx, const float* centers, void* ws,
                     int64_t ws_bytes, dmvae_gmm_result* out);

/* ---- k-means++ seeding of those centres on the device (csrc/gmm_seed.hip; Arthur & Vassilvitskii 2007, and the greedy form of
 * sklearn's _kmeans_plusplus), n_init restarts side by side --------------------------------------------------------------------
 * With T trials per centre (local_trials: 1 = plain D^2 sampling, 0 = sklearn's T = 2 + int(ln K), 2..8 = that many) and the uniforms
 * u [n_init][K][T] in [0, 1):
 *   centre 0 of restart r is row min(floor(u[r][0][0] * N), N - 1);  d2_n = ||x_n - c_0||^2 (f32 differences, summed over d ascending)
 *   centre k >= 1: tot = sum_n d2_n (f64, workgroup partials added in block order); candidate t is the first row whose f64 running
 *     sum of d2 (rows in order) exceeds u[r][k][t] * tot, never a row with d2 = 0 (tot not > 0: row min(floor(u * N), N - 1));
 *     the candidate with the smallest potential sum_n min(d2_n, ||x_n - cand_t||^2) is kept (the first on ties, as argmin), then
 *     d2_n = min(d2_n, ||x_n - c_k||^2).
 * u == NULL: u[i] = element i of the Philox stream (seed, step 0, stream id 3) of dmvae_philox_uniform.
 * centers [n_init][K][D] receive the chosen rows of X bit for bit, rows [n_init][K] (may be NULL) their indices.  After the call the first
 * n_init * K * T int32 of the workspace hold every round's candidate rows [n_init][K][T] (round 0: trial 0 only, the others -1).
 * No float atomics and no host synchronisation: 2 launches per centre with T = 1, else 2 + 3 (K - 1), all enqueued up front.
 * DMVAE_EINVAL: N, D, K, n_init < 1, K > N, local_trials outside 0..8, flags != 0, a workspace too small.  DMVAE_EUNSUPPORTED: T > 8
 * (local_trials = 0 with K >= 1097) or 4 * T * D + 4096 > 65536 bytes of LDS (the T candidate rows are staged there). */
typedef struct dmvae_gmm_seed_config {
    int32_t N, D, K;
    int32_t n_init;          /* restarts R >= 1                                     */
    int32_t local_trials;    /* 0: 2 + int(ln K); 1..8                              */
    uint64_t seed;           /* of the Philox stream when u is NULL                 */
    int32_t flags;           /* reserved: 0                                         */
} dmvae_gmm_seed_config;
int64_t dmvae_gmm_seed_ws_bytes(const dmvae_gmm_seed_config* cfg);      /* < 0: an error code */
int dmvae_gmm_seed(void* stream, const dmvae_gmm_seed_config* cfg, const float* X, int64_t ldx, const float* u, void* ws, int64_t ws_bytes,
                   float* centers, int32_t* rows);

/* ---- clustering evaluation (get_accuracy: base_models.py:425-432, 654-670, models.py:115-135; get_clustering_accuracy,
 * includes/utils.py:22-34) on the device (csrc/eval_clusters.hip) ---------------------------------------------------------
 * The confusion matrix the Hungarian step is solved on, built where the scores are: conf [R][R] int32, entry [cluster][class],
 * which the calls ADD INTO (the caller zeroes it once, runs every batch of the set, reads it back once).
 *   cluster of batch row r = the first index of the largest of its K scores (np.argmax's rule; the scores hold no NaN)
 *   class of batch row r   = classes[perm ? perm[first + r] : first + r]   (int32 [n_rows]; the indexing of dmvae_plan_load_batch)
 * Rows >= n_valid count nothing.  A class outside [0, R) counts nothing and sets bit 0 of *err_flag (device int32; the caller
 * checks it with the matrix), a perm entry outside [0, n_rows) bit 1.  Counts are integer atomics: exact in any order.
 * 1 <= K <= R <= 4096, 0 <= first, first + n_valid <= n_rows (DMVAE_EINVAL). */
int dmvae_confusion_add(void* stream, const float* scores, int64_t ld, int n_valid, int K, const int32_t* classes, int64_t n_rows,
                        const int32_t* perm, int64_t first, int32_t* conf, int R, int32_t* err_flag);
/* The same for the batch loaded by dmvae_plan_load_batch: dmvae_plan_encode, then
 *   DMVAE plans (MoE attachment or not): the count on the "logits" view, K = n_classes; draws / eps / eval_counter are ignored;
 *   VaDE plans: ONE encoder pass, then for j < draws in ascending order Z_j = mean + exp(log_var / 2) eps_j,
 *     gamma_j = get_cluster_probs(Z_j) (priors.py:91-102), w = (sum_j gamma_j) / draws -- written to the "eval_w" view
 *     [batch_pad][>= K], rows < n_valid -- and the count on w.  eps: device f32 [draws][n_valid][ld_eps], or NULL: Philox in the
 *     kernel, eps_j[r][d] = element ((j * n_rows + first + r) * latent_dim + d) of the stream (plan seed, step = eval_counter,
 *     stream id 2) of dmvae_philox_normal -- a function of the row's position in the evaluated order, not of the batch size.
 *     1 <= draws <= 1024.  The prior tables live in LDS as in the step's latent stage: the same limit, DMVAE_EUNSUPPORTED. */
int dmvae_plan_eval_clusters(dmvae_plan* p, void* stream, int n_valid, const int32_t* classes, int64_t n_rows, const int32_t* perm,
                             int64_t first, int draws, const float* eps, int64_t ld_eps, uint64_t eval_counter, int32_t* conf, int R,
                             int32_t* err_flag);

/* ---- held-out log-likelihood on the device (csrc/eval_loglik.hip): the importance-weighted bound of Burda et al. (2016) ------
 * For the batch loaded by dmvae_plan_load_batch (the f32 copy of the batch holds the targets: a dmvae_plan_load_batch_step batch is
 * refused), row r, draws s < S = draws, prior tables mu, lambda [K][D] (the same formula on DMVAE and VaDE plans: both hold a uniform
 * prior over the clusters):
 *   z_s = mean + exp(log_var / 2) eps_s                      (ONE encoder pass; bf16 plans: the decoder reads z_s rounded to bf16, the
 *                                                             prior and posterior terms the f32 z_s, as in the step)
 *   log q_s    = -1/2 sum_d (eps_sd^2 + log_var_d + log 2 pi)
 *   log p(z_s) = logsumexp_k [ -1/2 sum_d ((z_sd - mu_kd)^2 exp(-lambda_kd) + lambda_kd + log 2 pi) ] - log K
 *   log p(x | z_s), l = the decoder's logits of z_s:  binary  sum_{i < input_dim} (x_i l_i - max(l_i, 0) - log(1 + exp(-|l_i|)))
 *                                                     real    -1/2 sum_{i < input_dim} (x_i - l_i)^2 - input_dim / 2 log 2 pi
 *   w_s = log p(x | z_s) + log p(z_s) - log q_s,    L_r = logsumexp_s w_s - log S      (S = 1: an ELBO on the marginal mixture prior)
 * row_ll (device f32 [n_valid], may be NULL) receives L_r; acc (device double [2], ADDED INTO: the caller zeroes it once, runs every
 * batch of the set, reads it back once) gains sum_r L_r and n_valid.  No float atomics, fixed-order sums: two runs agree bit for bit.
 * eps: device f32 [draws][n_valid][ld_eps], or NULL: Philox in the kernel, eps_s[r][d] = element ((s * n_rows + first + r) * latent_dim + d)
 * of the stream (plan seed, step = eval_counter, stream id 4) of dmvae_philox_normal -- a function of the row's position in the
 * evaluated order, not of the batch size.  ws: the caller's scratch of dmvae_plan_eval_loglik_ws_bytes() bytes (host arithmetic on
 * batch_pad; the plan's own workspace does not grow).  Parameters, gradients, Adam moments and the step state are not written; the
 * "Z", "recon" (left holding the last draw's f32 logits) and decoder activation views are.  The prior tables pass through LDS in tiles: every K and latent_dim a plan can be
 * created with runs.  Every argument is checked before anything is enqueued; DMVAE_EINVAL: draws outside 1 .. 1024, first < 0,
 * first + n_valid > n_rows, n_valid > max_batch, ld_eps < latent_dim, a scratch too small, acc NULL. */
int64_t dmvae_plan_eval_loglik_ws_bytes(const dmvae_plan* p);
int dmvae_plan_eval_loglik(dmvae_plan* p, void* stream, int n_valid, int64_t n_rows, int64_t first, int draws, const float* eps,
                           int64_t ld_eps, uint64_t eval_counter, void* ws, int64_t ws_bytes, float* row_ll, double* acc);

/* ---- exact t-SNE of latent samples on the device (csrc/tsne.hip; the scatter of visualization.py:93-110, which the reference draws with
 * sklearn.manifold.TSNE(n_components=2)): sklearn's method="exact" with alpha = 1 and two output dimensions -------------------------
 * X [N][ldx] f32, D columns.
 *   d2_ij   = sum_d (x_id - x_jd)^2                      f32 differences, summed over d ascending (no norm expansion)
 *   p_{j|i} = exp(-beta_i d'_j) / s_i,  d'_j = d2_ij - min_{j != i} d2_ij,  s_i = sum_{j != i} exp(-beta_i d'_j),  p_{i|i} = 0
 *             beta_i: from 1, EXACTLY 64 bisection steps on H = log s + beta sum_j d'_j exp(-beta d'_j) / s against log(perplexity)
 *             (H > log u: lo = beta, beta doubles while no upper bound is known, else (beta + hi) / 2; otherwise hi = beta,
 *             beta = (beta + lo) / 2 with lo = 0 at first); s and the numerator are summed in f64.  No early exit: sklearn's search
 *             stops at |H - log u| <= 1e-5 within 100 steps, this one is a function of the data alone.
 *   P_ij    = (p_{j|i} + p_{i|j}) / 2N                   formed once per unordered pair: P == P^T bit for bit, zero diagonal, no floors
 *   gradient at Y [N][2] with exaggeration e:  q_ij = 1 / (1 + |y_i - y_j|^2), q_ii = 0, Z = sum_ij q_ij (f64, rows in a fixed order),
 *             g_i = 4 [ e sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_j q_ij^2 (y_i - y_j) ]
 *   step (sklearn's _gradient_descent, elementwise): inc = U g < 0; G = inc ? G + 0.2 : 0.8 G; G = max(G, 0.01);
 *             U = momentum U - learning_rate (G g); Y += U
 *   fit:      joint P; Y = Y0, or Y0 == NULL: Y[k] = 1e-4f * element k (k < 2N) of the Philox stream (seed, step 0, stream id 5) of
 *             dmvae_philox_normal; U = 0, G = 1; n_iter steps -- the first exaggeration_iters with e = early_exaggeration and
 *             momentum 0.5, the others with e = 1 and momentum 0.8 -- and KL = sum_{P_ij > 0} P_ij log(P_ij Z / q_ij) in f64 at the
 *             final Y.  ALL n_iter steps run: sklearn's n_iter_without_progress / min_grad_norm checks are left out.
 * dmvae_tsne_fit is dmvae_tsne_joint_p, then n_iter times what dmvae_tsne_step enqueues, then the KL: the same bits.
 * The workspace holds the dense [N][N] f32 matrix first (d2, then p_{j|i}, then P, in place: dmvae_tsne_p(ws) == ws) and O(N) behind
 * it; it must be 16-byte aligned, Y / U / G / grad / kl 8-byte aligned.  dmvae_tsne_gradient and dmvae_tsne_step need the P that
 * dmvae_tsne_joint_p left in the same workspace for the same config.  beta (device f32 [N], may be NULL) receives the beta_i.
 * No float atomics, fixed-order sums: two runs agree bit for bit.  The calls enqueue only -- 3 launches for the joint P, 3 per
 * step, 4 for the KL -- and never synchronise.  Every argument is checked before anything is enqueued; DMVAE_EINVAL: N < 4, D < 1,
 * perplexity outside (1, N - 1), n_iter or exaggeration_iters < 0, early_exaggeration or learning_rate not > 0, flags != 0, ldx < D,
 * a workspace too small or misaligned, a null pointer.  DMVAE_EUNSUPPORTED: N > 32768 (the matrix would pass 4 GiB). */
typedef struct dmvae_tsne_config {
    int32_t N, D;
    float perplexity;
    float early_exaggeration;
    float learning_rate;
    int32_t n_iter;
    int32_t exaggeration_iters;
    uint64_t seed;           /* of the Philox stream when Y0 is NULL                */
    int32_t flags;           /* reserved: 0                                         */
} dmvae_tsne_config;
int64_t dmvae_tsne_ws_bytes(const dmvae_tsne_config* cfg);      /* < 0: an error code */
int dmvae_tsne_joint_p(void* stream, const dmvae_tsne_config* cfg, const float* X, int64_t ldx, void* ws, int64_t ws_bytes, float* beta);
int dmvae_tsne_gradient(void* stream, const dmvae_tsne_config* cfg, void* ws, int64_t ws_bytes, const float* Y, float exaggeration, float* grad);
int dmvae_tsne_step(void* stream, const dmvae_tsne_config* cfg, void* ws, int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration,
                    float momentum);
int dmvae_tsne_fit(void* stream, const dmvae_tsne_config* cfg, const float* X, int64_t ldx, const float* Y0, void* ws, int64_t ws_bytes, float* Y,
                   double* kl);
const float* dmvae_tsne_p(const void* ws);

/* ---- kNN-sparse t-SNE on the device (csrc/tsne_knn.hip): the P of sklearn.manifold.TSNE(method="barnes_hut") with the repulsive term
 * kept EXACT over all pairs, for N up to 2^20 (no N x N array) -------------------------------------------------------------------------
 *   k       = min(N - 1, int(3 perplexity + 1)) <= 256, the cap of dmvae_knn (perplexity up to 85)
 *   lists   : idx / d2 [N][k] of dmvae_knn(X, X, k, self_first = 0), ordered by (d2, j)
 *   p_{j|i} = exp(-beta_i d'_t) / s_i over the row's k entries t, d'_t = d2[i][t] - d2[i][0], s_i = sum_t exp(-beta_i d'_t);
 *             beta_i by the search of the dense form above: from 1, EXACTLY 64 bisection steps, s and the numerator in f64
 *   P_ij    = (p_{j|i} + p_{i|j}) / 2N over the UNION of the lists, an absent direction counting 0, as CSR sorted by (row, column):
 *             indptr int64 [N + 1], indices int32 [nnz], values f32 [nnz]; P_ij and P_ji are the same bits.  The library leaves this
 *             one-off step to the caller (dmvae_hip/tsne.py: a stable sort of the int64 keys i N + j; a key occurs at most twice)
 *   gradient: g_i = 4 [ e sum_{j in row i} P_ij q_ij (y_i - y_j) - (1 / Z) sum_{j != i} q_ij^2 (y_i - y_j) ], Z = sum_{i != j} q_ij:
 *             the first sum over the CSR entries (a wave per row, lanes in entry order), the others over ALL pairs -- f32 sums inside
 *             a tile of <= 1024 columns, tiles joined in tile order (the q sum in f64), the columns dealt in whole tiles to S splits
 *             whose partials [S][N] are added in split order.  S = col_splits, or for 0: min(tiles, ceil(2048 / ceil(N / 256))).
 *   step, fit, KL: as the dense form, the KL over the CSR entries (f64 terms) with Z from one more all-pairs pass at the final Y.
 * dmvae_tsne_knn_fit is the start (Y0 or the Philox normals, as dmvae_tsne_fit), then n_iter times what dmvae_tsne_knn_step enqueues, then
 * the KL: the same bits.  The calls enqueue only -- 1 launch for the conditional p, 5 per step, 6 for the KL -- and read nothing back.
 * Every argument is checked before anything is enqueued; DMVAE_EINVAL: N outside 4 .. 2^20, perplexity outside (1, N - 1), k above 256
 * or not the k above, n_iter or exaggeration_iters < 0, early_exaggeration or learning_rate not > 0, col_splits outside 0 .. 64,
 * nnz < 0, flags != 0, ldd or ldp < k, a workspace too small or not 16-byte aligned, a null pointer.  Y / U / G / grad / kl / indptr
 * 8-byte aligned.  Entries of indptr outside [0, nnz] are clamped and columns outside [0, N) skipped: nothing outside the arrays is read. */
typedef struct dmvae_tsne_knn_config {
    int32_t N, k;
    int64_t nnz;             /* entries of the CSR (dmvae_tsne_knn_cond_p does not look at it) */
    float perplexity;
    float early_exaggeration;
    float learning_rate;
    int32_t n_iter;
    int32_t exaggeration_iters;
    int32_t col_splits;      /* 0: chosen from N                                     */
    uint64_t seed;           /* of the Philox stream when Y0 is NULL                */
    int32_t flags;           /* reserved: 0                                         */
} dmvae_tsne_knn_config;
int64_t dmvae_tsne_knn_ws_bytes(const dmvae_tsne_knn_config* cfg);      /* < 0: an error code */
int dmvae_tsne_knn_cond_p(void* stream, const dmvae_tsne_knn_config* cfg, const float* d2, int64_t ldd, float* p, int64_t ldp, float* beta);
int dmvae_tsne_knn_gradient(void* stream, const dmvae_tsne_knn_config* cfg, const int64_t* indptr, const int32_t* indices, const float* values,
                            void* ws, int64_t ws_bytes, const float* Y, float exaggeration, float* grad);
int dmvae_tsne_knn_step(void* stream, const dmvae_tsne_knn_config* cfg, const int64_t* indptr, const int32_t* indices, const float* values, void* ws,
                        int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration, float momentum);
int dmvae_tsne_knn_fit(void* stream, const dmvae_tsne_knn_config* cfg, const int64_t* indptr, const int32_t* indices, const float* values,
                       const float* Y0, void* ws, int64_t ws_bytes, float* Y, double* kl);

/* ---- cluster quality on the device (csrc/cluster_metrics.hip): the label of every row, and the silhouette coefficient of rows under
 * labels (Rousseeuw 1987; sklearn.metrics.silhouette_samples with the Euclidean metric).  The reference reports accuracy alone. ------
 * dmvae_argmax_labels: labels[r] (device int32 [n_valid]) = the first index of the largest of row r's K scores, scores [n_valid][ld]
 *   f32 -- np.argmax's rule, exact ties included, the rule of dmvae_confusion_add (the scores hold no NaN; what lies between the rows
 *   is not read).  1 <= K <= 4096, ld >= K, n_valid >= 0 (DMVAE_EINVAL).
 * dmvae_silhouette: Z [n][ldz] f32, D columns used (what lies between the rows is not read), labels device int32 [n] in [0, K):
 *   n_k  = rows with label k
 *   d_ij = sqrt(sum_c (z_ic - z_jc)^2)              f32 differences summed over c ascending (no norm expansion), correctly rounded sqrt
 *   a_i  = sum_{j: l_j = l_i} d_ij / (n_{l_i} - 1)
 *   b_i  = min over k != l_i with n_k > 0 of sum_{j: l_j = k} d_ij / n_k                      (empty clusters are skipped)
 *   s_i  = (b_i - a_i) / max(a_i, b_i);  0 when n_{l_i} = 1, when max(a_i, b_i) = 0, or when no other cluster has a row
 *   The rows of a cluster are summed in ascending row order; a running f32 sum takes at most 64 distances before it is added into a
 *   double; a, b and s are formed in double.  samples (device f32 [n]) receives s_i rounded to f32; out (device double
 *   [2], 8-byte aligned) receives out[0] = sum_i s_i, added in a fixed order, and out[1] = the number of non-empty clusters.  A label
 *   outside [0, K) sets bit 0 of *err_flag (device int32, OR-ed into: the caller zeroes it), and that row is left out of every sum and
 *   gets s = 0.  No float atomics, fixed-order sums: two calls on the same inputs return the same bits.  No N x N or N x K array is
 *   stored: ws is the caller's scratch of dmvae_silhouette_ws_bytes(n, K) bytes (host arithmetic, linear in n + K), 8-byte aligned.
 *   The call enqueues only (one memset and five launches) and never synchronises; every index into the rows is 64-bit.  Every argument
 *   is checked before anything is enqueued; DMVAE_EINVAL: n outside 2 .. 2^20, K outside 1 .. 4096, D < 1, ldz < D, a workspace too
 *   small or misaligned, a null Z / labels / samples / out / err_flag. */
int dmvae_argmax_labels(void* stream, const float* scores, int64_t ld, int n_valid, int K, int32_t* labels);
int64_t dmvae_silhouette_ws_bytes(int64_t n, int K);      /* < 0: an error code */
int dmvae_silhouette(void* stream, const float* Z, int64_t ldz, int n, int D, const int32_t* labels, int K, void* ws, int64_t ws_bytes,
                     float* samples, double* out, int32_t* err_flag);

/* ---- posterior diagnostics on the device (csrc/mixture_density.hip): the log-density of points under a diagonal
 * Gaussian mixture with any number of components, samples of the encoder posteriors, and the column statistics of the encoder outputs.
 * The reference has none of it.  Definitions, for rows n < N with encoder outputs mu_n and lv_n = log-variance (f32) and points i < M:
 *   z_i = mu_i + exp(lv_i / 2) eps_i
 *   a_i = log q(z_i | x_i) = -1/2 sum_d (eps_id^2 + lv_id) - (D/2) log 2 pi
 *   m_i = log q(z_i)       = logsumexp_j [ -1/2 sum_d ((z_id - mu_jd)^2 exp(-lv_jd) + lv_jd) ] - (D/2) log 2 pi - log N      (all N rows, j = i included)
 *   p_i = log p(z_i)       = the same over the K prior rows, - log K (the marginal mixture prior)
 *   mi = mean_i (a_i - m_i) <= mi_cap = log N (He et al. 2019);  marginal_kl = mean_i (m_i - p_i);  rate = mean_i (a_i - p_i) = mi + marginal_kl
 *   var_of_mean[d] = Var_n mu_nd (population);  mean_of_var[d] = mean_n exp(lv_nd);  active_units = #{d : var_of_mean[d] > threshold}
 * dmvae_mixture_logpdf: out[i] (device f32 [M]) = logsumexp_{j < J} (log_w[j] + log N(z_i; mu_j, diag exp(lv_j))), the -(D/2) log 2 pi
 *   included.  Z [M][ldz], mean [J][ldm], log_var [J][ldv] f32, D columns used, read where they are; log_w device f32 [J] or NULL =
 *   uniform weights, -log J.  An entry of -inf is a component of weight 0: it contributes nothing, also when it is the nearest one; if
 *   every entry is -inf the result is -inf.  Finite inputs never give NaN.  Arithmetic: exp(-lv) by __expf and c_j = log_w[j] - 1/2 sum_d
 *   lv_jd (the sum in double) are prepared into the workspace; the quadratic form in the DIFFERENCE form -- e = z - mu, e * e, fma with
 *   exp(-lv), d ascending in f32 (no norm expansion: it cancels at variances of 1e-6); t_ij = c_j - Q_ij / 2 in f32; the logsumexp as a running
 *   (max f32, sum f64) with one __expf per pair, the pairs joined in a fixed order; log in double, the constants added in double, one
 *   rounding to f32.  Per-point error bound, with w_ij the responsibilities and u = 2^-24:
 *     u [ (D + 5 + max |lv|) sum_j w_ij (Q_ij / 2 + 1/2 sum_d |lv_jd|) + 8 (|out_i| + 1) ]
 *   Few points against many components: J is split across workgroups into partial (max, sum) pairs in the workspace, joined by a second
 *   launch; the split is a function of (M, J, D) alone (dmvae_mixture_logpdf_split returns the number of parts: 1 when ceil(M / 16) >= 1024 or
 *   J <= 256).  Nothing read from ws depends on what it held before the call.  No float atomics: two calls return the same bits.  ws:
 *   dmvae_mixture_logpdf_ws_bytes(M, J, D) bytes (host arithmetic), 8-byte aligned.  Three or four launches, no synchronisation.  Every
 *   argument is checked before anything is enqueued; DMVAE_EINVAL: M or J outside 1 .. 2^20, D < 1, an ld < D, a workspace too small or
 *   misaligned, a null Z / mean / log_var / out.
 * dmvae_posterior_sample: Z[i] (f32 [n][ldz]) = z_i and logq[i] (f32 [n]) = a_i, formed in double and rounded once.  eps f32 [n][ld_eps], or
 *   NULL: Philox stream 6, step = counter, element philox_normal_at((pos0 + i) D + d).  0 <= pos0 <= 2^34.
 * dmvae_column_stats: out (device double [3][D], 8-byte aligned) = the column means of mu, var_of_mean, mean_of_var over the n rows, in
 *   double in a fixed order; the variance TWO-PASS (centred on the first pass's mean): a column at 1000 +- 1e-3 keeps its 1e-6
 *   variance, an all-equal column gives exactly 0.  ws: dmvae_column_stats_ws_bytes(n, D) bytes, 8-byte aligned.  Four launches.
 * dmvae_sum_f64: out[0] (device double, 8-byte aligned) = sum of x[0 .. n) (f32) in double, a fixed order.  One launch. */
int64_t dmvae_mixture_logpdf_ws_bytes(int64_t M, int64_t J, int64_t D);      /* < 0: an error code */
int dmvae_mixture_logpdf_split(int M, int J, int D);
int dmvae_mixture_logpdf(void* stream, const float* Z, int64_t ldz, int M, int D, const float* mean, int64_t ldm, const float* log_var, int64_t ldv,
                         int J, const float* log_w, void* ws, int64_t ws_bytes, float* out);
int dmvae_posterior_sample(void* stream, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, const float* eps,
                           int64_t ld_eps, uint64_t seed, uint64_t counter, int64_t pos0, float* Z, int64_t ldz, float* logq);
int64_t dmvae_column_stats_ws_bytes(int64_t n, int64_t D);                   /* < 0: an error code */
int dmvae_column_stats(void* stream, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, void* ws, int64_t ws_bytes,
                       double* out);
int dmvae_sum_f64(void* stream, const float* x, int64_t n, double* out);

/* ---- exact k-nearest neighbours on the device (csrc/knn.hip): kNN accuracy of the encoder means, the data rows nearest
 * a prior mean, the trustworthiness of an embedding.  The reference has none of it.  One distance and one order throughout:
 *   d2(i, j) = acc after  acc = fmaf(q_ic - x_jc, q_ic - x_jc, acc),  c = 0 .. D - 1 ascending, f32 differences, acc starting at 0 (no norm
 *              expansion: near rows do not cancel);  pairs of one query are ordered by (d2, j) ascending, a TOTAL order: an exact tie goes
 *              to the lower row.  The inputs are finite.
 * dmvae_knn: idx[i][0 .. k) (device int32 [M][ldo]) and d2[i][0 .. k) (f32 [M][ldo]) = the k rows of X [N][ldx] nearest row i of Q [M][ldq] in that
 *   order and their d2; D columns are used, what lies between the rows is not read, and nothing outside the k columns is written.
 *   self_first >= 0 leaves row self_first + i of X out of query i's neighbours (self-kNN, also of a slice of the queries); < 0 leaves nothing
 *   out.  Because the order is total the result is a function of the inputs alone.  ws: the caller's scratch of dmvae_knn_ws_bytes(M, N, D, k)
 *   bytes (host arithmetic; 0 when the queries alone fill the device: ws may then be NULL), 8-byte aligned.  One or two launches.
 *   DMVAE_EINVAL: M or N outside 1 .. 2^20, D < 1, k outside 1 .. 256, k > N - (self_first >= 0 ? 1 : 0), ldq < D, ldx < D, ldo < k, a workspace
 *   too small or misaligned, a null Q / X / idx / d2.
 * dmvae_knn_vote: counts[i][c] (f32 [M][ldc], c < C) = the number of query i's k neighbours idx[i][0 .. k) (int32 [M][ldi]) whose class
 *   classes[idx] (device int32 [N]) is c: exact small integers, so dmvae_argmax_labels on the counts is the uniform-weight vote (the smallest
 *   class among the tied ones) and dmvae_confusion_add takes them as scores.  An index outside [0, N) or a class outside [0, C) sets bit 0 of
 *   *err_flag (device int32, OR-ed into), checked before it indexes anything, and that neighbour counts nowhere.  1 <= C <= 4096, ldc >= C,
 *   ldi >= k.  One launch.
 * dmvae_knn_ranks: ranks[i][t] (int32 [N][ldr]) = #{l != i: (d2(i, l), l) < (d2(i, j), j)}, j = idx[i][t] (int32 [N][ldi], t < k): the 0-based rank of
 *   row j among row i's neighbours in X [N][ldx], all pairs -- the all-pairs half of sklearn.manifold.trustworthiness.  An index outside
 *   [0, N) or equal to i sets bit 0 of *err_flag and gets rank -1.  2 <= N <= 2^20, 1 <= k <= min(256, N - 1).  One launch.
 * All three only enqueue and never synchronise; every argument is checked before anything is enqueued (DMVAE_EINVAL with the error text
 * set); every index into the rows is 64-bit; no float atomics: two calls on the same inputs return the same bits. */
int64_t dmvae_knn_ws_bytes(int64_t M, int64_t N, int D, int k);             /* < 0: an error code */
int dmvae_knn(void* stream, const float* Q, int64_t ldq, int M, const float* X, int64_t ldx, int N, int D, int k, int64_t self_first, void* ws,
              int64_t ws_bytes, int32_t* idx, float* d2, int64_t ldo);
int dmvae_knn_vote(void* stream, const int32_t* idx, int64_t ldi, int M, int k, const int32_t* classes, int N, int C, float* counts, int64_t ldc,
                   int32_t* err_flag);
int dmvae_knn_ranks(void* stream, const float* X, int64_t ldx, int N, int D, const int32_t* idx, int64_t ldi, int k, int32_t* ranks, int64_t ldr,
                    int32_t* err_flag);

/* ---- sample quality on the device (csrc/prdc.hip): the all-pairs counts behind improved precision and recall
 * (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of generated rows against real rows.  The reference has none of it.
 * R [N][ldr] holds the real rows' features, F [M][ldf] the generated rows' (f32, unit column stride, D columns used; what lies between the
 * rows is not read).  d2(i, j) is THE distance of dmvae_knn above -- acc = fmaf(r_ic - f_jc, r_ic - f_jc, acc), f32 differences, c ascending, acc
 * starting at 0 -- from the same tile body, so its bits are those dmvae_knn returns; negating an f32 difference is exact, so d2(R_i, F_j) and
 * d2(F_j, R_i) are the same bits and one pass over the pairs serves both directions.  Radii are SQUARED distances and INPUTS (device f32):
 *   rR2[i] = the d2 of R_i's k-th nearest other real row, rF2[j] the same within F: column k - 1 of dmvae_knn(X, X, k, self_first = 0).
 * Balls are CLOSED: a pair is inside when d2 <= r2 -- the papers' definition (the `prdc` package compares with <, which differs at exact
 * ties only).  A radius may be +inf (every pair inside) and must not be NaN: that is not checked on the device.  Outputs (device memory):
 *   fake_in_real[j] (int32 [M]) = #{i : d2(i, j) <= rR2[i]}        real_in_fake[i] (int32 [N]) = #{j : d2(i, j) <= rF2[j]}
 *   real_min_d2[i]  (f32 [N])   = min_j d2(i, j)                   real_min_j[i]   (int32 [N], may be NULL) = its j, the lowest on a tie
 * from which, with the k the radii were taken at,
 *   precision = #{j : fake_in_real[j] > 0} / M        recall   = #{i : real_in_fake[i] > 0} / N
 *   density   = sum_j fake_in_real[j] / (k M)         coverage = #{i : real_min_d2[i] <= rR2[i]} / N.
 * fake_in_real is zeroed on the stream, then added into with integer atomics (integer addition commutes); the minimum is an integer
 * minimum on (d2, j) keys; there are no float atomics: two calls on the same inputs return the same bits.  One memset and one launch of
 * ceil(N / 16) workgroups -- both sets hold thousands of rows in every use; a small N is not split.  The call only enqueues and never
 * synchronises; every argument is checked before anything is enqueued (DMVAE_EINVAL with the entry's name in the error text: N or M outside
 * 1 .. 2^20, D < 1, ldr < D, ldf < D, a null R / F / rR2 / rF2 / fake_in_real / real_in_fake / real_min_d2); rows are indexed in 64 bits.
 * The model-level evaluation (get_sample_quality) draws its generated rows from Philox stream 7, step = counter,
 * element philox_normal_at(j D + d) of generated row j: ids 0 .. 6 are taken above. */
int dmvae_prdc_counts(void* stream, const float* R, int64_t ldr, int N, const float* F, int64_t ldf, int M, int D, const float* rR2,
                      const float* rF2, int32_t* fake_in_real, int32_t* real_in_fake, float* real_min_d2, int32_t* real_min_j);

/* ---- Sinkhorn divergence on the device (csrc/sinkhorn.hip): the softmin pass of the log-domain Sinkhorn iteration
 * behind the debiased entropic optimal-transport cost S_eps (Feydy et al. 2019; Genevay et al. 2018) between decoded prior draws and data.
 * The reference has none of it.  X [N][ldx] and Y [M][ldy] are f32 rows (unit column stride, D columns used; what lies between the rows is
 * not read).  The cost is C_ij = d2(X_i, Y_j), THE distance of dmvae_knn above -- acc = fmaf(x_c - y_c, x_c - y_c, acc), f32 differences, c
 * ascending, acc starting at 0 -- from the same tile body, so a pair's bits are those dmvae_knn returns.  No 1/2 factor: as eps -> 0,
 * S_eps -> the squared 2-Wasserstein distance.  With g (device f32 [M], NULL: zeros) the column potentials, log_b (device f32 [M], NULL:
 * -log M, the uniform weights; -inf: the column carries no mass) the column log-weights and eps > 0, all in f32 with 1 / eps rounded once:
 *   h_j  = fmaf(g_j, 1 / eps, log_b_j)        t_ij = fmaf(-d2_ij, 1 / eps, h_j)        out_i = -eps logsumexp_j t_ij      (device f32 [N])
 * the logsumexp as a running (maximum f32, scaled sum f64) with one f32 exponential per pair, -eps (m + log s) formed in double and rounded
 * once.  With prev (device f32 [N]) non-NULL the entry writes (prev_i + out_i) / 2 instead -- formed in double, rounded once: the averaged
 * update of the symmetric problems OT_eps(a, a).  A column with h_j = -inf never enters; a row whose columns are all empty gets +inf; no NaN
 * is formed from finite inputs, whatever the size of g / eps.  The solver (dmvae_hip.sinkhorn) alternates f <- softmin_Y(g), g <- softmin_X(f)
 * -- both this entry with the roles of X and Y swapped -- under an eps-scaling schedule; at a fixed point OT_eps = <a, f> + <b, g> and
 *   S_eps = sum_i a_i (f_i - p_i) + sum_j b_j (g_j - q_j),      p and q the potentials of the symmetric problems of a and b.
 * There are no float atomics: a workgroup owns 16 rows, walks every column, and joins its 256 partials per row in a fixed order, so two
 * calls on the same inputs return the same bits.  One launch of ceil(N / 16) workgroups, no workspace, no memset -- both sets hold thousands
 * of rows in every use; a small N is not split.  The call only enqueues and never synchronises; every argument is checked before anything is
 * enqueued (DMVAE_EINVAL with the entry's name in the error text: N or M outside 1 .. 2^20, D < 1, ldx < D, ldy < D, eps not finite, not
 * > 0 or so small that 1 / eps overflows f32, a null X / Y / out); rows are indexed in 64 bits. */
int dmvae_sinkhorn_softmin(void* stream, const float* X, int64_t ldx, int N, const float* Y, int64_t ldy, int M, int D, const float* g,
                           const float* log_b, float eps, const float* prev, float* out);

/* ---- binarised rows on the device (csrc/binarize.hip): the binarised-MNIST protocol of the literature on the resident
 * rows.  The reference has none of it: it feeds grey levels as soft Bernoulli targets.  X [n_rows][ldx] and out [n_rows][ldo]
 * are f32 rows (unit column stride, n_cols columns used; what lies between the rows of X is not read, what lies between the rows of out is
 * not written).  mode 0, the stochastic binarisation of Salakhutdinov & Murray 2008:
 *   out[r][c] = u(r, c) < X[r][c] ? 1 : 0,   u = word (idx & 3) of Philox block (idx >> 2) of stream 8 at (seed, step = counter), as the uniform
 *   (w >> 8) * 2^-24 in [0, 1),   idx = (row_base + r) * n_cols + c   in 64 bits,
 * row_base the index of row 0 of the call in the unpermuted data set: the draw of an element depends on (seed, counter, data-set row, column)
 * alone, so calls on chunks of the rows with their own row_base give what one call on all of them gives.  X = 0 never fires and X = 1 always
 * does; values outside [0, 1] are no error (below 0: 0; 1 or more: 1).  mode 1, the fixed binarisation by threshold: out = X > 0.5f ? 1 : 0,
 * no noise is read and seed / counter / row_base do not enter.  A NaN gives 0 in both modes.  One Philox block serves four consecutive idx, so
 * n_cols need not be a multiple of 4 and no padding is asked for.  The call only enqueues and never synchronises; every argument is checked
 * before anything is enqueued (DMVAE_EINVAL with the entry's name in the error text: a null X / out, n_rows < 1, n_cols < 1, ldx < n_cols,
 * ldo < n_cols, row_base < 0, a mode other than 0 / 1, (row_base + n_rows) * n_cols >= 2^58 -- the block index must stay below the stream bits
 * -- and out overlapping X: the byte spans of the two sides, first element to last, must be disjoint). */
int dmvae_binarize_rows(void* stream, const float* X, int64_t ldx, int64_t n_rows, int n_cols, int64_t row_base, uint64_t seed, uint64_t counter,
                        int mode, float* out, int64_t ldo);

/* ---- random affine augmentation of rows on the device (csrc/augment.hip).  The reference has none of it.  A row of
 * X [n_rows][ldx] (f32, unit column stride) is ONE single-plane image of H x W pixels, row-major (n_cols = H W; 1 <= H, W <= 64); out
 * [n_rows][ldo] gets its warp.  theta (six floats m00 m01 m02 m10 m11 m12 per row) is the SAMPLING map in pixel-index units, from output
 * pixel (row i, column j) to the source coordinate
 *   sx = m00 j + m01 i + m02,   sy = m10 j + m11 i + m12      (float32: fmaf(m00, j, fmaf(m01, i, m02)), and alike for sy),
 * and the output value is the bilinear interpolation of the source image extended by zeros -- each of the four taps outside [0, W) x [0, H)
 * contributes 0: torch's grid_sample(mode = "bilinear", padding_mode = "zeros", align_corners = True) after the unit conversion.  With
 * x0 = floor(sx), fx = sx - x0 (and y alike):  top = fmaf(fx, v01 - v00, v00), bot = fmaf(fx, v11 - v10, v10), out = fmaf(fy, bot - top, top).
 * A NaN or Inf coordinate gives 0.  Integer maps copy bits.
 * theta_in [n_rows][6] (device) gives the maps; with theta_in NULL they are DRAWN from p: uniforms of Philox stream 9 at (seed, step = counter),
 * blocks 2 g and 2 g + 1 with g = row_base + r, the row's index in the unpermuted data set -- so chunked calls with their own row_base equal
 * one call in bits, and batch size, row order and rank count do not enter.  u = (w >> 8) 2^-24, s = 2 u - 1.  Block 2 g, words 0 .. 3:
 * angle = rotate_deg s0, tx = translate_px s1, ty = translate_px s2, scale = exp(log lo + u3 (log hi - log lo)); block 2 g + 1, word 0:
 * shear = shear_deg s0 (words 1 .. 3 are reserved).  The forward transform acts about the centre c = ((W - 1) / 2, (H - 1) / 2),
 *   p_out = c + t + R(angle) Shear_x(tan shear) scale (p_in - c),
 * and theta is its inverse, formed in closed form on the device (csrc/augment.hip states the float32 order).  All-zero ranges with
 * scale (1, 1) give the identity and out == X in bits.  theta_out [n_rows][6] (device, or NULL) receives the maps used.  Pad columns of out
 * (H W <= c < ldo) are never written.  The call only enqueues and never synchronises; every argument is checked before anything is enqueued
 * (DMVAE_EINVAL with the entry's name in the error text: a null X / out; p and theta_in both null; n_rows < 1; H or W outside 1 .. 64;
 * ldx < H W; ldo < H W; row_base < 0; 2 (row_base + n_rows) >= 2^56; out overlapping X; and, when the maps are drawn, a range that is not
 * finite or is negative, scale_lo <= 0 or scale_lo > scale_hi). */
typedef struct dmvae_augment_params {
    float rotate_deg;     /* angle uniform in [-rotate_deg, rotate_deg) degrees */
    float translate_px;   /* tx, ty uniform in [-translate_px, translate_px) pixels */
    float scale_lo;       /* scale log-uniform in [scale_lo, scale_hi] */
    float scale_hi;
    float shear_deg;      /* shear angle uniform in [-shear_deg, shear_deg) degrees */
} dmvae_augment_params;
int dmvae_augment_rows(void* stream, const float* X, int64_t ldx, int64_t n_rows, int H, int W, int64_t row_base, uint64_t seed, uint64_t counter,
                       const dmvae_augment_params* p, const float* theta_in, float* theta_out, float* out, int64_t ldo);

/* ---- structural similarity on the device (csrc/ssim.hip): the SSIM of Wang et al. 2004 and the squared error of
 * n_pairs comparisons of image rows.  The reference has none of it.  Comparison r reads row X[ix ? ix[r] : r] and row Y[iy ? iy[r] : r]
 * (ix, iy: device int32 [n_pairs] or NULL; X and Y may be the same buffer).  A row is `planes` images of H x W f32, one after another; ldx,
 * ldy >= planes H W are the row strides, and what lies between the rows is never read.  The window is separable: the 2-D weight is
 * g[a][b] = fl32(w1[a] w1[b]); w1 is a HOST pointer to win floats, read at call time -- it travels in the kernel's argument struct and is not
 * kept.  win is odd, 3 <= win <= 11, win <= min(H, W).  Only windows that lie wholly inside the image count (VALID): for win = 11 and a
 * Gaussian of sigma 1.5 that is skimage's structural_similarity(gaussian_weights=True, use_sample_covariance=False), whose crop of
 * (win - 1) / 2 pixels never sees the padding.  Per window, in f32 with every product and sum rounded where it is written:
 *   mx = sum g x, my = sum g y                    acc = fmaf(g, x, acc), a ascending, b ascending inside it
 *   sxx = sum g (x - mx)^2, syy, sxy alike        acc = fmaf(g, fl(dx dy), acc): CENTRED on the window's own means; no E[x^2] - mu^2 anywhere
 *   S = (2 fl(mx my) + c1) (2 sxy + c2) / ((fl(mx mx) + fl(my my) + c1) (sxx + syy + c2))      the division correctly rounded
 * ssim[r] (device f32 [n_pairs]) = the mean of S over all windows of all planes (summed in f64, a fixed order); sse[r] (device f32
 * [n_pairs], may be NULL) = sum (x - y)^2 over the whole row -- a SUM, callers divide -- exact on rows of multiples of 1/16.  Two
 * properties hold in BITS because the sequence is pinned: ssim(X, X) == 1.0f, and ssim(X, Y) == ssim(Y, X).  There are no atomics on
 * floats; a wave owns a comparison and sums in a fixed order, so two calls return the same bits.  An ix / iy entry outside [0, nx) /
 * [0, ny) reads nothing: NaN goes to that comparison's outputs and bit 1 of *err_flag (device int32, OR-ed into, may be NULL) is set.
 * One launch, no memset; the call only enqueues and never synchronises; every argument is checked before anything is enqueued, with the
 * entry's name in the error text.  DMVAE_EINVAL: a null X / Y / ssim / w1; n_pairs, nx, ny, H, W or planes < 1; win even, outside 3 .. 11
 * or above min(H, W); ldx or ldy below planes H W.  DMVAE_EUNSUPPORTED: H W > 4096 (the two planes of a pair are held in 32 KiB of LDS).
 * Rows are indexed in 64 bits. */
int dmvae_ssim_rows(void* stream, const float* X, int64_t ldx, int64_t nx, const int32_t* ix, const float* Y, int64_t ldy, int64_t ny,
                    const int32_t* iy, int64_t n_pairs, int H, int W, int planes, const float* w1, int win, float c1, float c2, float* ssim,
                    float* sse, int32_t* err_flag);

/* ---- linear probe of the latent means on the device (csrc/probe.hip): one evaluation of the multinomial logistic
 * regression (softmax regression) loss and gradient over all rows -- the hot path of an L-BFGS fit -- and the scores of a fitted probe.  The
 * reference has none of it.  With u = 2^-24, Z [n][ldz] f32, classes int32 [n], W [D][ldw], b [C] (all device memory):
 *   x_id = (Z_id - shift_d) * scale_d in f32; shift and scale (f32 [D]) are both NULL -- x is then Z bit for bit -- or both given;
 *   l_ic = b_c + sum_d x_id W_dc, accumulated in f32 by fmaf over d ascending, starting from b_c;   m_i = max_c l_ic;
 *   loss_i = log sum_c exp(l_ic - m_i) + m_i - l_{i, y_i}   (the log-sum-exp form: finite when the true class's probability underflows);
 *   p_ic = exp(l_ic - m_i) / sum_c exp(l_ic - m_i);   r_ic = p_ic - [c = y_i].
 * dmvae_softmax_xent: out (device double [1 + D C + C], 8-byte aligned, ONE buffer so that one copy brings everything back) =
 *   out[0] = (1 / n) sum_i loss_i;  gW[d][c] = out[1 + d C + c] = (1 / n) sum_i x_id r_ic;  gb[c] = out[1 + D C + c] = (1 / n) sum_i r_ic.
 *   No penalty term: the caller adds it in float64.  Per-row terms (x, l, p, r, loss_i) are f32; a workgroup adds its rows in ascending order
 *   in f64, the workgroups' partials are added in f64 in a fixed order; the slabs are a function of (n, D, C) alone and there are no float
 *   atomics, so two calls return the same bits.  A class outside [0, C) ORs bit 0 into *flag (device int32) before it indexes anything; that
 *   row adds nothing to any sum and the divisor stays n.  ws: the caller's scratch of dmvae_softmax_xent_ws_bytes(n, D, C) bytes (host
 *   arithmetic), 8-byte aligned.  Two launches.
 * dmvae_linear_scores: scores[i][c] (f32 [M][lds], c < C) = l_ic of the rows of Z [M][ldz], by the device function the loss kernel uses for x
 *   and for l: the same bits.  Nothing outside the C columns is written.  dmvae_argmax_labels on the scores is the prediction (a tie to the
 *   smaller class) and dmvae_confusion_add takes them.  One launch.
 * Domain: 1 <= n, M <= 2^22, 1 <= D <= 512, 2 <= C <= 256, D C <= 16384 (W and b, padded, take at most 70 KiB of LDS beside a row tile), ldz >= D,
 *   ldw >= C, lds >= C.  Both only enqueue and never synchronise; every argument is checked before anything is enqueued (DMVAE_EINVAL with the
 *   entry's name in the error text: outside the domain, a null Z / classes / W / b / out / flag / scores, one of shift and scale alone, a
 *   workspace too small or misaligned); rows are indexed in 64 bits. */
int64_t dmvae_softmax_xent_ws_bytes(int64_t n, int D, int C);               /* < 0: an error code */
int dmvae_softmax_xent(void* stream, const float* Z, int64_t ldz, int64_t n, int D, const float* shift, const float* scale, const int32_t* classes, int C,
                       const float* W, int64_t ldw, const float* b, void* ws, int64_t ws_bytes, double* out, int32_t* flag);
int dmvae_linear_scores(void* stream, const float* Z, int64_t ldz, int M, int D, const float* shift, const float* scale, const float* W, int64_t ldw,
                        const float* b, int C, float* scores, int64_t lds);

/* ---- label spreading on a sparse symmetric graph (csrc/label_spread.hip): the hot path of the few-label evaluator
 * (Zhou et al. 2004, Learning with local and global consistency).  The reference has none of it.  The graph W is CSR on the device -- indptr
 * int64 [N + 1], indices int32 [nnz] ascending within a row, values f32 [nnz] -- symmetric and without a diagonal: what the union of the lists
 * of dmvae_knn(X, X, k, self_first = 0) gives.  Whatever indptr holds, only entries [0, nnz) are read.
 * dmvae_graph_sym_normalize: d_i = sum_j W_ij in float64 in CSR order, r_i = d_i^-1/2 rounded once to f32 (exactly 0 for a row without edges;
 *   r f32 [N]), s_ij = (W_ij r_i) r_j in f32 (s f32 [nnz], the layout of w).  A column index outside [0, N) ORs bit 0 into *err_flag (device
 *   int32); that entry adds nothing to d_i, gets s = 0 and nothing is read through it.  Two launches.
 * dmvae_label_spread: n_iter >= 1 iterations F <- alpha S F + (1 - alpha) Y, one launch each, Y the one-hot of labels (device int32 [N], -1:
 *   no label) over C classes.  Per element acc = fmaf(s_ij, F[j][c], acc) over the row's entries ascending, from 0, then
 *   F'[i][c] = fmaf(alpha, acc, (1 - alpha) [labels_i == c]) with 1 - alpha rounded once: a function of the inputs alone, whatever the launch
 *   shape.  F_in (device f32 [N][ld_in], ld_in >= C; NULL: zeros) is the start -- the F of an earlier call, the same buffer included, continues
 *   it bit for bit; the result lands in F [N][ldf], ldf >= C, whose columns >= C keep their bits.  change[t] (device f32 [n_iter]) =
 *   max_ic |F^(t+1) - F^t|, joined from per-wave maxima in integer order (no float atomics; a NaN in F gives a NaN); nothing past n_iter entries
 *   is written.  A label outside {-1} u [0, C) ORs bit 1 into *err_flag and the row counts as unlabelled; a column index outside [0, N) ORs bit 0
 *   and the entry is skipped.  ws: the caller's scratch of dmvae_label_spread_ws_bytes(N, C) bytes (host arithmetic), 16-byte aligned: two
 *   copies of F with C padded to a multiple of 4 and the per-wave maxima.  No host synchronisation, no cooperative launch, no spinning: the
 *   kernel boundary is the only ordering between workgroups.
 * Domain: 1 <= N <= 2^20, 2 <= C <= 1024, 0 < alpha < 1, any row degree.  Both only enqueue; every argument is checked before anything is
 * enqueued (DMVAE_EINVAL with the entry's name in the error text); rows are indexed in 64 bits; two calls return the same bits. */
int dmvae_graph_sym_normalize(void* stream, const int64_t* indptr, const int32_t* indices, const float* w, int N, int64_t nnz, float* s, float* r,
                              int32_t* err_flag);
int64_t dmvae_label_spread_ws_bytes(int64_t N, int C);                     /* < 0: an error code */
int dmvae_label_spread(void* stream, const int64_t* indptr, const int32_t* indices, const float* s, int N, int64_t nnz, const int32_t* labels, int C,
                       float alpha, int n_iter, const float* F_in, int64_t ld_in, float* F, int64_t ldf, float* change, void* ws, int64_t ws_bytes,
                       int32_t* err_flag);

/* Measurement and tuning entry points (per-kernel timing for bench.py's roofline leg, probes, tile knobs) are
 * declared in dmvae_hip_debug.h: exported by the same library, not part of the drop-in boundary. */
int dmvae_abi_version(void);
const char* dmvae_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DMVAE_HIP_H */
