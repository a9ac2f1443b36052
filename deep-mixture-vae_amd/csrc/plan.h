// The step plan as the host files see it (plan.hip, step.hip, eval.hip, api.hip): layers, ACTIVATION DESCRIPTORS, the plan itself,
// and the few host functions the files share.  No device code.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "kernels.h"

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

struct PLayer {
    std::string name;
    int in, out, in_pad, out_pad;
    int64_t w_off, b_off, ldw;    // arena element offsets; ldw = row stride of W
};

// One 3x3 SAME convolution of the CNN trunk (base_models.py:181-201), as the GEMMs it runs as (conv.hip).
// Activations are zero-bordered: [Bp][P][P][ld] (P = hw + 2) with P + 1 zero guard rows on either end; an
// o_* offset points at the guard, rows0() at padded pixel 0.
struct PConv {
    std::string name;
    int cin, cout, hw, pool;          // channels, image side of its input = output, 2x2 SAME max-pool behind it
    int cin_ld, cout_ld;              // channel stride of the input / output activation: the channel count itself (32, 64, 128; the image: 1)
    int cin_np, cout_np;              // channels padded to 64 = N of the GEMM that produces such an activation, ld of the weight matrix
    int P;                            // hw + 2
    int kdim, ktdim;                  // K of the forward / input-gradient GEMM: 9 * cin / 9 * cout padded to 64 (first layer: an explicit 9-column patch matrix)
    int64_t w_off, b_off;             // W [kdim][cout_ld]: HWIO flattened, rows (tap, c < cin), zero pad rows / columns; b [cout_ld]
    int64_t o_act, o_dact;            // relu output and its gradient
    int64_t o_pool, o_dpool;          // pooled output (zero-bordered for the next conv; the last one plain = the flat trunk output) and its gradient
};

// One [Bp][cols] activation of the plan's workspace.  dmvae_plan_create (the MoE buffers: dmvae_plan_attach_moe) is the ONLY place that
// states a buffer's shape; every GEMM helper, evaluator and view reads it from here.  es is per buffer: mean | log_var, the logits, the
// responsibilities, gmu / glv / clv, the reconstruction ... are f32 on bf16 plans too.
struct PAct {
    int64_t off = -1;                 // workspace byte offset (-1: this plan has no such buffer)
    int cols = 0;                     // columns of this view (padded)
    int64_t ld = 0;                   // leading dimension in elements
    int es = 4;                       // bytes per element
    // bias gradients of the macro-tile path: the GEMM that PRODUCES a dY (256x256 kernel, ReLU-gate / recon epilogue) leaves its column sums
    // per 256-row tile, [Bp/256][ld] floats at byte offset cs (of THESE columns; -1: none); the dW problem of that layer picks them up
    int64_t cs = -1;
    mutable bool cs_live = false;     // this pass: the producer of the WHOLE tensor was the macro tile and has left them (cleared by forward_and_loss)
    const PAct* whole = nullptr;      // of a column range: the descriptor it was cut from (cs_live is kept there)

    // columns [c0, c0 + n): the z / c halves of hzc and dhzc, the log_var half of mv.  Its column-sum slot moves with it.
    PAct sub(int c0, int n) const {
        PAct v = *this;
        v.off += (int64_t)c0 * es; v.cols = n; v.cs_live = false; v.whole = whole ? whole : this;
        if (cs >= 0) v.cs += (int64_t)c0 * 4;
        return v;
    }
    void mark_cs_live() const { (whole ? whole : this)->cs_live = true; }
};

struct dmvae_plan {
    dmvae_config cfg;
    std::vector<PConv> conv;          // cfg.trunk == DMVAE_TRUNK_CNN only
    int flat = 0;                     // 4*4*128 = 2048: width of the flattened pool output feeding enc0
    int64_t o_wt = 0, o_c0part = 0, o_cslab = 0;     // o_cslab: K-slice slabs of the conv weight gradients (cfg.deterministic)
    int64_t conv_param_end = 0;
    int Bp, Ip, Dp, Kp, Hp, Tp;   // padded batch / input / latent / classes / head / trunk
    int es;                        // bytes per activation element
    std::vector<PLayer> enc, dec;
    PLayer zc, mv, lg, out;        // fused z|c hidden, fused mean|log_var, logits, output layer
    int64_t prior_off;             // prior_means [K][D] then prior_log_vars [K][D], contiguous
    int64_t tail_off = 0;          // [tail_off, param_elems): every bias, then the prior tables -- the tensors the epilogues and the
                                   // latent kernel read in fp32 (0.3 % of the arena), kept apart from the weight matrices
    int64_t param_elems;
    std::vector<dmvae_tensor_info> tensors;
    // activations (act: the plan's dtype; the others f32).  x: the act copy of the batch, xf its f32 copy (an f32 plan: the same buffer), x2:
    // the second bf16 batch buffer (see pf); cflat / dflat: the CNN trunk's flattened pool output and its gradient
    struct {
        PAct x, xf, x2, cflat, dflat, hzc, mv, lg, Z, Zf, gmu, glv, clv, w, dlg, recon, dl, dmv, dhzc;
        std::vector<PAct> enc, dec, denc, ddec;
    } a;
    // scratch (byte offsets; not activations: loss / prior-gradient partials, the bias-gradient slab sums, the MFMA latent forms' scratch)
    int64_t o_rpart, o_lpart, o_dprior, o_cs, o_lws = 0;
    int64_t lws_bytes = 0;            // scratch of the MFMA form of the latent contractions (0: the one-kernel form)
    // K slices of the thin dense launches of a SMALL batch (ksplit_for): slabs of f32 partial tiles + one ticket per tile (zero between launches)
    int64_t o_ksws = -1, ksws_elems = 0, o_ktick = -1;
    int n_rpart, n_lblk, n_pblk;      // loss-partial blocks of the latent kernel; rows of its prior-table gradient partials (as of plan creation)
    int n_lblk_cap = 0;               // rows the partial-sum buffers hold
    int64_t cs_elems;
    int64_t work_bytes;
    dmvae_buffers buf;
    bool bound;
    std::vector<dmvae::GemmArgs> dw_queue;   // dW problems queued (bf16: flushed as grouped launches)
    // Large batches (Bp >= 8192, MNIST-shaped layers): the dW group's tile count is fixed by the parameter shapes while its K = the
    // batch grows -- few, very long workgroups (cfg3: 256 K tiles each) that fill the CUs' slots unevenly and re-fetch their operand
    // panels (1.75x at cfg3, profiles/r03_cfg3_pmc_traffic.txt).  Then every problem is cut into dw_slices K slices, each a set of
    // ordinary workgroups of the SAME grouped launch storing its partial product (and bias partial) into its own slab -- a full image
    // of the gradient arena per slice, [dw_slices_max][param_elems] floats at o_dwslab -- and the slabs are added in ascending order
    // by the Adam kernel (adam_slabs: fused step) or by slab_reduce into the gradient arena (backward alone).  No float atomics.
    int dw_slices_max = 1;            // 1: the plan has no slabs
    int64_t o_dwslab = 0;
    int dw_slices_now = 1;            // slices of the pass being enqueued
    bool dw_macro_now = false;        // ... and whether its 256-divisible layers take the macro tile (their bias gradient: a bias-only strip)
    int dw_macro_tiles = 0;           // 256x256 tiles of those layers (per K slice)
    bool fused_update = false;        // set for the duration of dmvae_plan_train_step on a bf16 plan
    bool staged = false;              // dmvae_plan_forward_backward_stage: every segment launches its own dW group
    int stage_groups = 3;             // ... or (2) segments 0 and 1 share one: dmvae_plan_set_stage_groups
    // dmvae_plan_load_batch_step: the batch was assembled for a step that follows at once -- no f32 copy of it exists; the output
    // layer's reconstruction epilogue reads its targets from the dataset through the same permutation (bf16 plans whose output
    // layer runs on the small-tile kernel, input_dim a multiple of 4)
    struct { const float* data; int64_t n_rows; const int32_t* perm; int64_t first; int n_valid; const void* st; } tsrc{};
    bool tsrc_valid = false;          // cleared by dmvae_plan_load_batch (which writes the f32 copy)
    bool tsrc_used = false;           // a forward pass has consumed that batch: the device cursor has moved on (step_finalize), so a second
                                      // pass without a reload would pair the old bf16 batch with the NEXT batch's targets -- refused
    bool tgt_gather = false;          // the plan is eligible
    // dmvae_plan_prefetch_batch: the NEXT batch is assembled while this step runs -- by workgroups riding in the trunk's dX launch where that
    // launch leaves them CUs of their own (place_riders), else by a gather launch of its own -- into the OTHER of two bf16 batch
    // buffers (x / x2); dmvae_plan_swap_batch then makes it the current one.  The step itself no longer starts with a gather.
    int xsel = 0;                     // the current batch buffer
    struct { const float* data; int64_t n_rows; const int32_t* perm; int64_t first; int n_valid; const void* st; bool armed, done; dmvae::dmvae_gather_args gat; } pf{};
    bool vade = false;                // cfg.model == DMVAE_MODEL_VADE: no head hidden layers, no logits; latent mode 2
    // mixture-of-experts attachment (dmvae_plan_attach_moe, models.py:10-163 of the reference): W_moe is the last weight matrix,
    // b_moe the last bias of the tail; the workspace grows by the buffers below.  Plans without it keep their layout.
    struct {
        bool on = false;
        dmvae_moe_config cfg{};
        int EO = 0, EOp = 0;
        PLayer L;                         // in = input_dim (featLearn off) or latent_dim (featLearn on), out = E * O
        PAct P, dP, inp, dq, pred, acc;   // expert outputs (f32), their gradient (act), the row kernel's input copy (act), its dq scratch, predictions, accumulators
        int64_t o_part = 0;
        int nblk = 0;
        const int32_t* perm = nullptr; int64_t first = 0; const void* st = nullptr;     // the batch's rows (recorded by the batch loads)
    } moe;
    // semi-supervised label attachment (dmvae_plan_attach_labels): the cross-entropy stage of label_xent.hip behind the latent stage.  No
    // parameter, no GEMM problem; the workspace grows by the three buffers below.  The batch's rows are the ones moe.perm / first / st record.
    struct {
        bool on = false;
        const int32_t* labels = nullptr; int64_t rows = 0;
        int64_t o_ctl = 0, o_acc = 0, o_err = 0;     // "label_ctl" (f32: [0] = w), "label_acc" (float64 [acc_elems]), "label_err" (int32)
        int64_t acc_elems = 0;
    } lab;
};

static inline int pad64(int x) { return (x + 63) / 64 * 64; }
static inline char* WS(const dmvae_plan* p, int64_t off) { return reinterpret_cast<char*>(p->buf.work) + off; }
static inline char* WS(const dmvae_plan* p, const PAct& a) { return WS(p, a.off); }
template <class X> static inline float* WSf(const dmvae_plan* p, const X& x) { return reinterpret_cast<float*>(WS(p, x)); }
// weights as seen by the GEMMs: bf16 shadow or the f32 master
static inline const void* Wp(const dmvae_plan* p, int64_t off) {
    return p->cfg.dtype == DMVAE_BF16 ? (const void*)(reinterpret_cast<const bf16_t*>(p->buf.param_bf16) + off)
                                      : (const void*)(p->buf.param + off);
}
static inline const PAct& XB(const dmvae_plan* p, int other = 0) { return ((p->xsel ^ other) && p->a.x2.off >= 0) ? p->a.x2 : p->a.x; }     // the current (other = 1: the next) act copy of the batch
// pointer to padded pixel 0 of a zero-bordered activation (skips the P + 1 guard rows)
static inline char* rows0(const dmvae_plan* p, int64_t off, int P, int ld) { return WS(p, off) + (int64_t)(P + 1) * ld * p->es; }

// What dmvae_latent_args (the step), VadeEvalArgs (eval_clusters) and LoglikDrawArgs (eval_loglik) all read: the posterior, the prior tables, the noise.
template <class A> static inline void latent_inputs(const dmvae_plan* p, A& a, const float* eps, int64_t ld_eps) {
    a.B_pad = p->Bp; a.D = p->cfg.latent_dim; a.K = p->cfg.n_classes;
    a.mean = WSf(p, p->a.mv); a.ld_mean = p->a.mv.ld;
    a.log_var = WSf(p, p->a.mv.sub(p->Dp, p->Dp)); a.ld_log_var = p->a.mv.ld;
    a.prior_means = p->buf.param + p->prior_off;
    a.prior_log_vars = a.prior_means + (int64_t)p->cfg.n_classes * p->cfg.latent_dim;
    a.eps = eps; a.ld_eps = ld_eps; a.seed = p->cfg.seed;
}
// ... and the sample they write (the step, eval_loglik): Z in the plan's dtype, and in f32 beside it on bf16 plans
template <class A> static inline void latent_sample(const dmvae_plan* p, A& a) {
    a.Z_act = WS(p, p->a.Z); a.ld_Z = p->a.Z.ld;
    a.Z_f32 = p->cfg.dtype == DMVAE_BF16 ? WSf(p, p->a.Zf) : nullptr; a.ld_Zf = p->a.Zf.ld;
}

namespace dmvae {
// api.hip
int gemm_checked(hipStream_t s, int dtype, int layout, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb,
                 const dmvae_epilogue* epi, int split, GemmArgs* deferred = nullptr, int conv_p = 0, int conv_c = 0);
int gemm_partials(int dtype, int M, int N);      // RECON loss partials live on the 64x64 cell grid of the output whatever tile a kernel uses
// step.hip
constexpr int KSPLIT_MAX_ROWS = 256, KSPLIT_MAX_SLICES = 8;      // K slices of thin dense launches (ksplit_for): batches of at most this many rows
bool step_set_knob(int which, int value);        // knobs 10, 11, 12, 16, 17, 21: false = not one of the step's
int fwd_dense(dmvae_plan* p, hipStream_t s, const PAct& in, const PLayer& L, int kind, const PAct& out, GemmArgs* deferred = nullptr);
int encode_impl(dmvae_plan* p, hipStream_t s, bool heads = true);
int decode_hidden(dmvae_plan* p, hipStream_t s);
int moe_stage(dmvae_plan* p, hipStream_t s, int n_valid, float inv_B, bool backward);
int label_stage(dmvae_plan* p, hipStream_t s, int n_valid, float inv_B);
int conv_dw_split(int64_t K, int tiles);
int conv_layer_dw(hipStream_t s, int dt, int M, int P, int cin, int kdim, const void* in, int64_t cin_ld, const void* dact, int64_t cout_ld,
                  int cout_np, int cout, int sp, float* slab, float* dW, float* db);
}  // namespace dmvae
