// The launch sequence of one session.run([loss, train_step]) on a plan (plan.h): batch assembly, the dense helpers (a layer + activation
// views in, one GEMM out), the CNN trunk, the weight-gradient queue, and the forward + backward pass as named segments.
#include <algorithm>

#include "plan.h"
#include "moe_head.h"
#include "label_xent.h"
#include "measure.h"

using namespace dmvae;

// tuning knob (dmvae_debug_set_knob 10): K slices of the dense weight-gradient group (0 = the plan's rule, 1 = none, 2 / 4 = forced where
// the plan has the slabs); see dmvae_plan::dw_slices_max
static int g_dw_slices = 0;
// tuning knob (dmvae_debug_set_knob 11): with K slices, the layers whose shape divides by 256 on the macro tile (1, default) or every
// layer on the small tiles (0)
static int g_dw_macro = 1;
static int g_pf_rides = 1;                  // tuning knob (dmvae_debug_set_knob 17): a prefetched batch's gather rides in the dZ GEMM where it has the room (1), or is a launch of its own (0)
static int g_fin_rides = 1;                 // tuning knob (dmvae_debug_set_knob 16): the step_finalize blocks ride in the dZ GEMM where it has the room, else in the heads' dX launch
                                            // (1, default); always in the heads' dX launch (2); a launch of their own (0)
static int g_heads_dx_form = 0;             // tuning knob (dmvae_debug_set_knob 12): the dX of the two head layers as one grouped launch (0 / 1) or as two launches (2)
static int g_ksplit = 1;                    // tuning knob (dmvae_debug_set_knob 21): 1 = the rule of ksplit_for, 0 = never
bool dmvae::step_set_knob(int which, int value) {
    int* const k = which == 10 ? &g_dw_slices : which == 11 ? &g_dw_macro : which == 12 ? &g_heads_dx_form : which == 16 ? &g_fin_rides :
                   which == 17 ? &g_pf_rides : which == 21 ? &g_ksplit : nullptr;
    if (k) *k = value;
    return k != nullptr;
}

// ====================================================================== batch assembly
// records the batch's rows for the MoE stage and drops a pending prefetch (every batch load)
static void batch_rows(dmvae_plan* p, const int32_t* perm, int64_t first, const void* st) {
    p->pf.armed = p->pf.done = false;
    p->moe.perm = perm; p->moe.first = first; p->moe.st = st;
}
extern "C" int dmvae_plan_load_batch(dmvae_plan* p, void* stream, const float* data, int64_t n_rows, const int32_t* perm,
                                     int64_t first, int n_valid, int use_state_cursor) {
    DMVAE_REQUIRE(p && p->bound && data, "dmvae_plan_load_batch: plan not bound / null data");
    DMVAE_REQUIRE(n_valid >= 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_load_batch: n_valid=%d exceeds max_batch=%d", n_valid, p->cfg.max_batch);
    void* xa = p->cfg.dtype == DMVAE_BF16 ? (void*)WS(p, XB(p)) : nullptr;
    p->tsrc_valid = false;
    batch_rows(p, perm, first, use_state_cursor ? p->buf.state : nullptr);
    return gather_launch((hipStream_t)stream, p->cfg.dtype, data, n_rows, p->cfg.input_dim, perm, first, p->cfg.max_batch, n_valid, p->Bp, xa, p->Ip,
                         WSf(p, p->a.xf), p->Ip, p->Ip, use_state_cursor ? p->buf.state : nullptr);
}

// The same for a caller that goes straight on to dmvae_plan_forward_backward / _train_step (one step on this batch, nothing else
// reads it).  On an eligible plan (tgt_gather) only the bf16 copy of the batch is written: the f32 copy's one reader in a step,
// the reconstruction epilogue of the output layer, fetches its target rows from `data` through `perm` itself -- the same bytes
// read, 4 B per input element less written and re-read (cfg2: the gather 9.9 -> 6 us).  The "x" view is then NOT valid.
// Otherwise exactly dmvae_plan_load_batch.  `data` / `perm` must stay alive and unchanged until the step has run.
extern "C" int dmvae_plan_load_batch_step(dmvae_plan* p, void* stream, const float* data, int64_t n_rows, const int32_t* perm,
                                          int64_t first, int n_valid, int use_state_cursor) {
    DMVAE_REQUIRE(p && p->bound && data, "dmvae_plan_load_batch_step: plan not bound / null data");
    DMVAE_REQUIRE(n_valid >= 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_load_batch_step: n_valid=%d exceeds max_batch=%d", n_valid, p->cfg.max_batch);
    if (!p->tgt_gather) return dmvae_plan_load_batch(p, stream, data, n_rows, perm, first, n_valid, use_state_cursor);
    p->tsrc.data = data; p->tsrc.n_rows = n_rows; p->tsrc.perm = perm; p->tsrc.first = first; p->tsrc.n_valid = n_valid;
    p->tsrc.st = use_state_cursor ? p->buf.state : nullptr;
    p->tsrc_valid = true;
    p->tsrc_used = false;
    batch_rows(p, perm, first, p->tsrc.st);
    if constexpr (MEAS_NO_STEP_GATHER) {      // measurement build 11 only (measure.h): timing of a step without its gather
        static int calls = 0;
        if (++calls > 2) return 0;
    }
    return gather_launch((hipStream_t)stream, DMVAE_BF16, data, n_rows, p->cfg.input_dim, perm, first, p->cfg.max_batch, n_valid, p->Bp,
                         WS(p, XB(p)), p->Ip, nullptr, p->Ip, p->Ip, use_state_cursor ? p->buf.state : nullptr);
}

// Arms the assembly of the NEXT batch inside the next forward + backward pass (see dmvae_plan::pf); with use_state_cursor the rows are those
// of the device cursor AFTER that pass's step_finalize has advanced it.  Needs a current batch assembled by dmvae_plan_load_batch_step (or
// made current by dmvae_plan_swap_batch) on an eligible plan; `data` / `perm` must stay alive and unchanged until the step that CONSUMES the
// prefetched batch has run (the step after the one that assembles it: that step's reconstruction epilogue still reads the targets through them).
extern "C" int dmvae_plan_prefetch_batch(dmvae_plan* p, const float* data, int64_t n_rows, const int32_t* perm, int64_t first, int n_valid,
                                         int use_state_cursor) {
    DMVAE_REQUIRE(p && p->bound && data, "dmvae_plan_prefetch_batch: plan not bound / null data");
    DMVAE_REQUIRE(n_valid >= 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_prefetch_batch: n_valid=%d exceeds max_batch=%d", n_valid, p->cfg.max_batch);
    if (p->moe.on) { set_error("dmvae_plan_prefetch_batch: not with a MoE attachment (its labels follow the current batch)"); return DMVAE_EUNSUPPORTED; }
    if (!p->tgt_gather || p->a.x2.off < 0) { set_error("dmvae_plan_prefetch_batch: this plan assembles its batches with dmvae_plan_load_batch (f32, conv trunk, or an output layer on the macro tile)"); return DMVAE_EUNSUPPORTED; }
    DMVAE_REQUIRE(p->tsrc_valid && !p->tsrc_used, "dmvae_plan_prefetch_batch: no current batch (dmvae_plan_load_batch_step or dmvae_plan_swap_batch first)");
    p->pf.data = data; p->pf.n_rows = n_rows; p->pf.perm = perm; p->pf.first = first; p->pf.n_valid = n_valid;
    p->pf.st = use_state_cursor ? p->buf.state : nullptr;
    p->pf.armed = true; p->pf.done = false;
    return 0;
}
// Makes the batch a pass has prefetched the current one (host state only: the other batch buffer and its target source).
extern "C" int dmvae_plan_swap_batch(dmvae_plan* p) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_swap_batch: plan not bound");
    DMVAE_REQUIRE(p->pf.done, "dmvae_plan_swap_batch: no pass has run since dmvae_plan_prefetch_batch");
    p->xsel ^= 1;
    p->tsrc.data = p->pf.data; p->tsrc.n_rows = p->pf.n_rows; p->tsrc.perm = p->pf.perm; p->tsrc.first = p->pf.first; p->tsrc.n_valid = p->pf.n_valid;
    p->tsrc.st = p->pf.st;
    p->tsrc_valid = true; p->tsrc_used = false;
    p->moe.perm = p->pf.perm; p->moe.first = p->pf.first; p->moe.st = p->pf.st;      // the current batch's rows (the label stage reads them)
    p->pf.armed = p->pf.done = false;
    return 0;
}

// ====================================================================== dense helpers
// K slices for the thin dense launches of a small batch.  At 100 rows (the reference's own default, train.py:215-216) every GEMM of the
// step is 2 x N / 64 tiles -- a few CUs, each walking the whole K chain and streaming its own weight panel: the launch lasts as long as that chain
// (K = 4096: 64 K tiles, 18 us).  Cut into S slices the chain is S times shorter on S times the CUs; the slices' partial tiles meet in a fixed-order
// sum by the last one to arrive (GemmArgs::tick): deterministic, no float atomics, no extra launch.  Returns S (1 = none).
static int ksplit_for(const dmvae_plan* p, int N, int K, int epi) {
    if (!g_ksplit || p->o_ksws < 0 || p->Bp > KSPLIT_MAX_ROWS || p->cfg.dtype != DMVAE_BF16 || K < 2048) return 1;
    if (epi != DMVAE_EPI_BIAS_RELU && epi != DMVAE_EPI_RELU_MASK && epi != DMVAE_EPI_BIAS_F32 && epi != DMVAE_EPI_LATENT) return 1;
    const int tiles = (epi == DMVAE_EPI_LATENT ? (p->Bp + 15) / 16 : p->Bp / 64) * (N / 64);      // (the dZ GEMM runs on 16-row tiles; a slab is sized for a 64 x 64 tile either way)
    int S = std::min(KSPLIT_MAX_SLICES, K / (g_ksplit == 2 ? 256 : 512));      // (knob 21 = 2: slices of 256 instead of 512)
    while (S > 1 && (K % (S * 64) || tiles * S > 256 || (int64_t)tiles * S * 4096 > p->ksws_elems)) --S;
    return tiles <= 64 ? std::max(S, 1) : 1;      // (a launch that already covers a quarter of the chip keeps its K chain)
}
// S > 1 K slices of a problem: their slabs and tickets
static void kslice(const dmvae_plan* p, GemmArgs& a, int S) {
    a.k_split = a.K / S;
    a.ws = WSf(p, p->o_ksws); a.ws_elems = p->ksws_elems;
    a.tick = reinterpret_cast<int*>(WS(p, p->o_ktick));
}
// a dense problem of the plan with its K slices, if the rule gives it any
static int gemm_plan(dmvae_plan* p, hipStream_t s, int layout, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, const dmvae_epilogue* e,
                     GemmArgs* deferred) {
    const int S = deferred ? 1 : ksplit_for(p, N, K, e->kind);
    if (S == 1) return gemm_checked(s, p->cfg.dtype, layout, p->Bp, N, K, A, lda, B, ldb, e, 1, deferred);
    GemmArgs a;
    TRY(gemm_checked(s, p->cfg.dtype, layout, p->Bp, N, K, A, lda, B, ldb, e, 1, &a));
    if (gemm_bf16_256_ok(layout, e->kind, p->Bp, N, K, false)) return gemm_bf16_dispatch(s, layout, a, 1);
    kslice(p, a, S);
    return gemm_bf16_dispatch(s, layout, a, S);
}

// out = epilogue(in . W + b) of layer L
int dmvae::fwd_dense(dmvae_plan* p, hipStream_t s, const PAct& in, const PLayer& L, int kind, const PAct& out, GemmArgs* deferred) {
    DMVAE_REQUIRE(in.cols == L.in_pad && out.cols == L.out_pad, "fwd_dense %s: views of %d -> %d columns on a %d -> %d layer", L.name.c_str(), in.cols, out.cols, L.in_pad, L.out_pad);
    dmvae_epilogue e;
    memset(&e, 0, sizeof(e));
    e.kind = kind; e.out = WS(p, out); e.ldo = out.ld; e.bias = p->buf.param + L.b_off;
    return gemm_plan(p, s, DMVAE_GEMM_FWD, L.out_pad, L.in_pad, WS(p, in), in.ld, Wp(p, L.w_off), L.ldw, &e, deferred);
}

static int launch_dw_queue(dmvae_plan* p, hipStream_t target, bool with_prior);

// dW = X^T dY into the grad arena, db = colsum(dY).  Split-K of the dW GEMMs: off.  Measured (tools/gemm_sweep.py) fp32-atomic split-K
// loses on every dW shape of the step except 512x512 (-13 %), so dW is a plain store and the whole step is bit-reproducible;
// cfg.deterministic is kept in the ABI for a future slab-reduce split-K.
static int grad_dense(dmvae_plan* p, hipStream_t s, const PAct& x, const PAct& dy, const PLayer& L) {
    DMVAE_REQUIRE(x.cols == L.in_pad && dy.cols == L.out_pad, "grad_dense %s: views of %d / %d columns on a %d -> %d layer", L.name.c_str(), x.cols, dy.cols, L.in_pad, L.out_pad);
    dmvae_epilogue e;
    memset(&e, 0, sizeof(e));
    const int nsl = p->cfg.dtype == DMVAE_BF16 ? p->dw_slices_now : 1;      // K slices into slabs (dw_slices_max)
    float* gbase = nsl > 1 ? WSf(p, p->o_dwslab) : p->buf.grad;
    e.kind = nsl > 1 ? DMVAE_EPI_STORE_F32 : p->fused_update ? DMVAE_EPI_ADAM : DMVAE_EPI_STORE_F32;
    e.out = gbase + L.w_off; e.ldo = L.ldw;
    e.out2 = gbase + L.b_off;             // db = column sums of dY, fused (ones-operand MFMA)
    if (p->cfg.dtype != DMVAE_BF16) return gemm_checked(s, p->cfg.dtype, DMVAE_GEMM_DW, L.in_pad, L.out_pad, p->Bp, WS(p, x), x.ld, WS(p, dy), dy.ld, &e, 1);
    // bf16: queued, all dW problems of the step go out as ONE grouped launch
    if ((int)p->dw_queue.size() >= DMVAE_MAX_GROUP) TRY(launch_dw_queue(p, s, false));    // deep stacks: a full group goes out early
    GemmArgs a;
    TRY(gemm_checked(s, DMVAE_BF16, DMVAE_GEMM_DW, L.in_pad, L.out_pad, p->Bp, WS(p, x), x.ld, WS(p, dy), dy.ld, &e, 1, &a));
    a.ws = WSf(p, p->o_cs); a.ws_elems = p->cs_elems;     // bias-gradient slab sums of a 256x256-tile problem
    if (nsl > 1) { a.k_split = p->Bp / nsl; a.slab_stride = a.slab_stride2 = p->param_elems; }       // slice y -> slab y (gemm_bf16_body)
    if (nsl > 1 && p->dw_macro_now && gemm_bf16_256_slice_ok(L.in_pad, L.out_pad, p->Bp / nsl)) {
        // this layer's slices run on the macro tile (gemm_bf16.hip peel_large_dw); the macro tile has no ones-operand pass, so the
        // bias gradient comes from a bias-only strip of the grouped small-tile launch: same K slices, same slabs
        GemmArgs b = a;
        b.M = 64; b.bias_only = 1;
        a.epi.out2 = nullptr;
        p->dw_queue.push_back(b);
    }
    if (dy.cs_live && dy.cols == dy.ld) {      // ... unless dY's producer left its column sums (PAct::cs)
        a.csum_in = WSf(p, dy.cs); a.csum_ld = dy.cols; a.csum_rows = p->Bp / 256;
    }
    p->dw_queue.push_back(a);
    return 0;
}

// Launch the queued weight-gradient problems as ONE grouped grid (with the Adam update in its
// epilogue under dmvae_plan_train_step).  Whole pass: everything queues until the last call (group 2) -- one launch;
// staged (dmvae_plan_forward_backward_stage, data parallel): every group is launched where it is flushed, so that its gradient
// bucket is final when the segment ends.  (The groups on a side stream beside the dX chain were measured twice and removed:
// 0.4235 vs 0.391 ms in round 1, 0.358 vs 0.292 ms in round 2 -- a fork / join pair in a replayed graph costs 15-20 us.)
static int flush_dw(dmvae_plan* p, hipStream_t s, int group) {
    if (p->dw_queue.empty()) return 0;
    if (!p->staged && group != 2) return 0;
    if (p->staged && p->stage_groups == 2 && group == 0) return 0;      // two launches: segment 0's problems go out with segment 1's
    return launch_dw_queue(p, s, group == 2);
}

// the queued problems as K slices into slabs, then the slabs' fixed-order sum: inside the Adam kernel (fused step) or into the gradient arena
static int launch_dw_slabs(dmvae_plan* p, hipStream_t target, bool with_prior) {
    const float* slab = WSf(p, p->o_dwslab);
    // the group's WEIGHT range and its BIAS range (the biases live in the arena tail, behind every weight matrix): kept apart,
    // because under the staged backward the span between them belongs to other segments -- buckets whose collective may
    // already be in flight (earlier segments) or whose gradients are not written yet (later ones)
    int64_t wlo = p->param_elems, whi = 0, blo = p->param_elems, bhi = 0;
    for (auto& a : p->dw_queue) {
        const int64_t w0 = reinterpret_cast<const float*>(a.epi.out) - slab;
        wlo = std::min(wlo, w0);
        whi = std::max(whi, w0 + (int64_t)a.M * a.epi.ldo);
        if (a.epi.out2) {
            const int64_t b0 = reinterpret_cast<const float*>(a.epi.out2) - slab;
            blo = std::min(blo, b0);
            bhi = std::max(bhi, b0 + (int64_t)a.N);
        }
    }
    const int64_t lo = std::min(wlo, blo), hi = std::max(whi, bhi);
    const int rc = gemm_bf16_grouped_dw(target, p->dw_queue.data(), (int)p->dw_queue.size());
    p->dw_queue.clear();
    if (rc) return rc;
    if (p->fused_update) {
        DMVAE_REQUIRE(with_prior && lo == 0, "dW slabs: the fused step flushes ONE group holding every layer");
        AdamArgs a;
        a.n = p->param_elems; a.p = p->buf.param; a.g = p->buf.grad; a.m = p->buf.m; a.v = p->buf.v;
        a.pb = reinterpret_cast<bf16_t*>(p->buf.param_bf16);
        a.lr = 0.f; a.b1 = p->cfg.beta1; a.b2 = p->cfg.beta2; a.eps = p->cfg.adam_eps; a.gscale = 1.f;
        a.zero_grad = 0; a.ieee = p->cfg.adam_ieee;
        a.t_host = ~0ull;                                   // t = state->adam_t, advanced by this step's step_finalize
        a.st = reinterpret_cast<const dmvae_state*>(p->buf.state);
        // [hi, param_elems): the prior tables (gradient complete in the arena, written by step_finalize) and the arena's zero tail
        return adam_slabs_launch(target, a, slab, p->dw_slices_now, p->param_elems, hi, p->param_elems);
    }
    if (!p->staged || bhi <= blo || blo <= whi)       // whole pass: every layer is in this group, the span between is only the tail's alignment pad (zeros)
        return slab_reduce_launch(target, slab + lo, hi - lo, p->dw_slices_now, p->param_elems, p->buf.grad + lo);
    // staged (data parallel): this segment's weights and this segment's biases, nothing in between (one reduce over
    // [lo, hi) rewrote the weight gradients of EARLIER segments -- whose reduce-scatter / all-reduce was already running -- with
    // local sums, and wrote stale slab values over biases that later segments had yet to produce)
    TRY(slab_reduce_launch(target, slab + wlo, whi - wlo, p->dw_slices_now, p->param_elems, p->buf.grad + wlo));
    return slab_reduce_launch(target, slab + blo, bhi - blo, p->dw_slices_now, p->param_elems, p->buf.grad + blo);
}

// one grouped launch of whatever is queued; with_prior: also the prior tables' Adam (once per fused step)
static int launch_dw_queue(dmvae_plan* p, hipStream_t target, bool with_prior) {
    if (p->dw_queue.empty()) return 0;
    if (p->dw_slices_now > 1) return launch_dw_slabs(p, target, with_prior);
    int rc;
    if (p->fused_update) {    // dmvae_plan_train_step: the Adam update rides in the epilogue of this launch
        dmvae_adam_ctx c;
        memset(&c, 0, sizeof(c));
        c.param = p->buf.param; c.grad = p->buf.grad; c.m = p->buf.m; c.v = p->buf.v; c.param_bf16 = p->buf.param_bf16;
        c.state = p->buf.state; c.beta1 = p->cfg.beta1; c.beta2 = p->cfg.beta2; c.epsilon = p->cfg.adam_eps; c.grad_scale = 1.f;
        c.store_grad = 0;
        c.ieee = p->cfg.adam_ieee;
        c.seg_off = p->prior_off;                       // prior tables: gradient written by step_finalize
        c.seg_n = with_prior ? ((2 * (int64_t)p->cfg.n_classes * p->cfg.latent_dim + 3) & ~(int64_t)3) : 0;
        rc = gemm_bf16_grouped_dw_adam(target, p->dw_queue.data(), (int)p->dw_queue.size(), c);
    } else {
        rc = gemm_bf16_grouped_dw(target, p->dw_queue.data(), (int)p->dw_queue.size());
    }
    p->dw_queue.clear();
    return rc;
}

// dx = (dy . W^T of layer L) gated by y_fwd > 0.  Where the 256x256 kernel runs it and dx has a column-sum slot (PAct::cs), the kernel
// leaves dx's column sums there for the weight-gradient problem of the layer that produced y_fwd (grad_dense).
// riders: the caller has asked gemm_bf16_riders_room -- a small-tile launch.
static int dx_dense(dmvae_plan* p, hipStream_t s, const PAct& dy, const PLayer& L, const PAct& y_fwd, const PAct& dx, GemmArgs* deferred = nullptr,
                    const GemmRiders* riders = nullptr) {
    DMVAE_REQUIRE(dy.cols == L.out_pad && y_fwd.cols == L.in_pad && dx.cols == L.in_pad, "dx_dense %s: views of %d -> %d / %d columns on a %d -> %d layer",
                  L.name.c_str(), dy.cols, y_fwd.cols, dx.cols, L.in_pad, L.out_pad);
    dmvae_epilogue e;
    memset(&e, 0, sizeof(e));
    e.kind = DMVAE_EPI_RELU_MASK; e.out = WS(p, dx); e.ldo = dx.ld; e.aux0 = WS(p, y_fwd); e.ld0 = y_fwd.ld;
    const int N = L.in_pad, K = L.out_pad, dt = p->cfg.dtype;
    const bool macro = !deferred && dx.cs >= 0 && dt == DMVAE_BF16 && gemm_bf16_256_ok(DMVAE_GEMM_DX, DMVAE_EPI_RELU_MASK, p->Bp, N, K, false);
    if (!riders && !macro) return gemm_plan(p, s, DMVAE_GEMM_DX, N, K, WS(p, dy), dy.ld, Wp(p, L.w_off), L.ldw, &e, deferred);
    GemmArgs a;
    TRY(gemm_checked(s, dt, DMVAE_GEMM_DX, p->Bp, N, K, WS(p, dy), dy.ld, Wp(p, L.w_off), L.ldw, &e, 1, &a));
    if (riders) return gemm_bf16_dispatch(s, DMVAE_GEMM_DX, a, 1, riders);
    a.csum_out = WSf(p, dx.cs); a.csum_ld = dx.ld;
    dx.mark_cs_live();
    return gemm_bf16_dispatch(s, DMVAE_GEMM_DX, a, 1);
}

// ====================================================================== CNN trunk
// CNN trunk forward (base_models.py:176-216) into the flat view.  First layer (one input channel): a direct kernel; every other
// convolution is ONE conv-mode GEMM straight off the zero-bordered activation (conv.hip) + bias + ReLU, then
// the border rows (which computed relu(bias)) are re-zeroed; SAME max-pools behind conv1 / conv3 / conv5.
static int conv_trunk_forward(dmvae_plan* p, hipStream_t s) {
    const int dt = p->cfg.dtype;
    const void* in = nullptr;                       // zero-bordered input of the next convolution, at padded pixel 0
    for (size_t i = 0; i < p->conv.size(); ++i) {
        const PConv& L = p->conv[i];
        const int M = p->Bp * L.P * L.P;
        dmvae_epilogue e;
        memset(&e, 0, sizeof(e));
        e.kind = DMVAE_EPI_BIAS_RELU; e.out = rows0(p, L.o_act, L.P, L.cout_ld); e.ldo = L.cout_ld; e.bias = p->buf.param + L.b_off;
        e.n_valid = L.cout;                          // a 32-channel output is stored 32 wide: the GEMM's other 32 columns are dropped
        if (i == 0) {   // one input channel: direct kernel, writes the border rows as zeros itself
            TRY(conv_first_fwd_launch(s, dt, WS(p, p->a.x), p->Ip, L.hw, p->Bp, Wp(p, L.w_off), L.cout_np, p->buf.param + L.b_off, L.cout,
                                      rows0(p, L.o_act, L.P, L.cout_ld), L.cout_ld));
        } else {
            TRY(gemm_checked(s, dt, DMVAE_GEMM_FWD, M, L.cout_np, L.kdim, in, L.cin_ld, Wp(p, L.w_off), L.cout_np, &e, 1, nullptr, L.P, L.cin));
            TRY(zero_border_launch(s, dt, rows0(p, L.o_act, L.P, L.cout_ld), L.P, L.cout_ld, p->Bp));
        }
        in = rows0(p, L.o_act, L.P, L.cout_ld);
        if (L.pool) {
            const bool last = i + 1 == p->conv.size();
            const int Po = (L.hw + 1) / 2 + 2;
            void* out = last ? (void*)WS(p, L.o_pool) : (void*)rows0(p, L.o_pool, Po, L.cout_ld);
            TRY(maxpool2_fwd_launch(s, dt, in, L.hw, L.cout_ld, p->Bp, out, last ? 0 : 1));
            in = out;
        }
    }
    return 0;
}

// largest split of K that keeps K-slices whole multiples of 64 and long enough to amortise a tile
int dmvae::conv_dw_split(int64_t K, int tiles) {
    const int64_t units = K / 64;
    int64_t target = std::min<int64_t>(units / 16, std::max(1, 2048 / std::max(1, tiles)));
    for (int64_t d = std::max<int64_t>(1, target); d >= 8; --d)       // a multiple of 8: one XCD per slice (gemm_bf16_kernel)
        if (units % d == 0 && d % 8 == 0) return (int)d;
    for (int64_t d = std::max<int64_t>(1, target); d > 1; --d)
        if (units % d == 0) return (int)d;
    return 1;
}

// Weight and bias gradient of ONE conv-mode layer (every convolution but the first): dW[kdim][cout_np] = X_patches^T dY, db = column sums of dY,
// over M padded pixel rows.  sp = 1: fp32 atomics into dW / db, which the caller has zeroed.  sp > 1: K slice y stores its partial product (and
// bias-gradient partial) into slab y of `slab` (sp * (kdim + 1) * cout_np floats); the slabs are then added in ascending order: bit-reproducible,
// no float atomics (the atomic form drifts after a few Adam steps).  Rows past the ninth tap are padding (the GEMM fills them with a copy of
// tap 8) and are zeroed last.  Called by conv_trunk_backward and by dmvae_debug_conv_dw (tests/test_gpu_conv_kernels.py).
int dmvae::conv_layer_dw(hipStream_t s, int dt, int M, int P, int cin, int kdim, const void* in, int64_t cin_ld, const void* dact, int64_t cout_ld,
                         int cout_np, int cout, int sp, float* slab, float* dW, float* db) {
    dmvae_epilogue e;
    memset(&e, 0, sizeof(e));
    e.kind = DMVAE_EPI_ATOMIC_F32; e.ldo = cout_np; e.n_valid = cout;
    e.out = dW; e.out2 = db;
    if (sp > 1) {
        const int64_t wn = (int64_t)kdim * cout_np;
        e.kind = DMVAE_EPI_STORE_F32; e.out = slab; e.out2 = slab + (int64_t)sp * wn;
        GemmArgs g;
        TRY(gemm_checked(s, dt, DMVAE_GEMM_DW, kdim, cout_np, M, in, cin_ld, dact, cout_ld, &e, 1, &g, P, cin));
        g.k_split = M / sp; g.slab_stride = wn; g.slab_stride2 = cout_np;
        if (dt == DMVAE_BF16) TRY(gemm_bf16_dispatch(s, DMVAE_GEMM_DW, g, sp));
        else {
            ProfScope ps(s, "gemm_f32_dw", 2.0 * g.M * g.N * (double)g.K, 4.0 * ((double)g.M * g.K + (double)g.K * g.N + (double)g.M * g.N));
            TRY(gemm_f32_dispatch(s, DMVAE_GEMM_DW, g, sp));
        }
        TRY(slab_reduce_launch(s, slab, wn, sp, wn, dW));
        TRY(slab_reduce_launch(s, slab + (int64_t)sp * wn, cout_np, sp, cout_np, db));
    } else
    TRY(gemm_checked(s, dt, DMVAE_GEMM_DW, kdim, cout_np, M, in, cin_ld, dact, cout_ld, &e, sp, nullptr, P, cin));
    if (kdim > 9 * cin) {
        const hipError_t me = hipMemsetAsync(dW + (int64_t)9 * cin * cout_np, 0, (size_t)(kdim - 9 * cin) * cout_np * 4, s);
        if (me != hipSuccess) { set_error("conv gradient pad memset: %s", hipGetErrorString(me)); return (int)me; }
    }
    return 0;
}

// CNN trunk backward from dflat (gradient of the flattened pool output).  Per layer, last to first:
//   un-pool + ReLU gate (maxpool2_bwd_relu)  ->  dY, zero-bordered;
//   dW: ONE DW-layout GEMM with M = (tap, channel): a tile row reads the layer's input shifted by its tap's row
//       offset, against dY over all padded rows (split-K, fp32 atomics into the zeroed gradient range); db rides along;
//   d(input): ONE conv-mode GEMM of dY with the flipped kernel, gated by the input activation's ReLU (which
//       also zeroes the border rows: the activation is zero there).
static int conv_trunk_backward(dmvae_plan* p, hipStream_t s) {
    const int dt = p->cfg.dtype;
    hipError_t me = hipMemsetAsync(p->buf.grad + p->conv.front().w_off, 0, (size_t)(p->conv_param_end - p->conv.front().w_off) * 4, s);
    if (me != hipSuccess) { set_error("conv gradient memset: %s", hipGetErrorString(me)); return (int)me; }
    for (int i = (int)p->conv.size() - 1; i >= 0; --i) {
        const PConv& L = p->conv[i];
        const int M = p->Bp * L.P * L.P;
        const bool last = i + 1 == (int)p->conv.size();
        char* dact = rows0(p, L.o_dact, L.P, L.cout_ld);
        if (L.pool) {
            const int Po = (L.hw + 1) / 2 + 2;
            const void* dpool = last ? (const void*)WS(p, p->a.dflat) : (const void*)rows0(p, L.o_dpool, Po, L.cout_ld);
            TRY(maxpool2_bwd_relu_launch(s, dt, rows0(p, L.o_act, L.P, L.cout_ld), dpool, L.hw, L.cout_ld, p->Bp, dact, last ? 0 : 1));
        }
        if (i == 0) {
            TRY(conv_first_dw_launch(s, dt, WS(p, p->a.x), p->Ip, L.hw, p->Bp, dact, L.cout_ld, L.cout, p->buf.grad + L.w_off, L.cout_np, p->buf.grad + L.b_off,
                                     WSf(p, p->o_c0part)));
            break;
        }
        const PConv& Lp = p->conv[i - 1];
        const char* in = Lp.pool ? rows0(p, Lp.o_pool, L.P, L.cin_ld) : rows0(p, Lp.o_act, L.P, L.cin_ld);
        TRY(conv_layer_dw(s, dt, M, L.P, L.cin, L.kdim, in, L.cin_ld, dact, L.cout_ld, L.cout_np, L.cout,
                          conv_dw_split(M, (L.kdim / 64) * (L.cout_np / 64)), WSf(p, p->o_cslab), p->buf.grad + L.w_off, p->buf.grad + L.b_off));
        TRY(conv_wflip_launch(s, dt, Wp(p, L.w_off), L.cin, L.cin_np, L.cout, L.cout_np, WS(p, p->o_wt), L.ktdim));
        dmvae_epilogue e;
        memset(&e, 0, sizeof(e));
        e.kind = DMVAE_EPI_RELU_MASK; e.ldo = L.cin_ld; e.aux0 = in; e.ld0 = L.cin_ld; e.n_valid = L.cin;
        e.out = Lp.pool ? rows0(p, Lp.o_dpool, L.P, L.cin_ld) : rows0(p, Lp.o_dact, L.P, L.cin_ld);
        TRY(gemm_checked(s, dt, DMVAE_GEMM_DX, M, L.cin_np, L.ktdim, dact, L.cout_ld, WS(p, p->o_wt), L.ktdim, &e, 1, nullptr, L.P, L.cout));
    }
    return 0;
}

// ====================================================================== encoder, decoder, MoE stage
// the encoder's input: the current batch buffer, or the CNN trunk's flattened pool output
static inline const PAct& trunk_input(const dmvae_plan* p) { return p->conv.empty() ? XB(p) : p->a.cflat; }

// heads = false: stop behind the [z|c]-hidden layer (the step then runs the two head layers inside the latent launch: heads_latent.hip)
int dmvae::encode_impl(dmvae_plan* p, hipStream_t s, bool heads) {
    const auto& a = p->a;
    if (!p->conv.empty()) TRY(conv_trunk_forward(p, s));
    const PAct* in = &trunk_input(p);
    for (size_t i = 0; i < p->enc.size(); ++i) {
        TRY(fwd_dense(p, s, *in, p->enc[i], DMVAE_EPI_BIAS_RELU, a.enc[i]));
        in = &a.enc[i];
    }
    if (p->vade) return fwd_dense(p, s, *in, p->mv, DMVAE_EPI_BIAS_F32, a.mv);      // VaDE: [mean | log_var] straight off the trunk (base_models.py:501-507), no logits
    TRY(fwd_dense(p, s, *in, p->zc, DMVAE_EPI_BIAS_RELU, a.hzc));
    if (!heads) return 0;
    // the two head layers [mean|log_var] = hz.Wmv and logits = hc.Wl are independent siblings:
    // bf16 issues them as one grouped grid (each alone is 64..128 workgroups)
    GemmArgs q[2];
    const bool grp = p->cfg.dtype == DMVAE_BF16;
    TRY(fwd_dense(p, s, a.hzc.sub(0, p->Hp), p->mv, DMVAE_EPI_BIAS_F32, a.mv, grp ? &q[0] : nullptr));
    TRY(fwd_dense(p, s, a.hzc.sub(p->Hp, p->Hp), p->lg, DMVAE_EPI_BIAS_F32, a.lg, grp ? &q[1] : nullptr));
    if (grp) TRY(gemm_bf16_grouped(s, DMVAE_GEMM_FWD, q, 2));
    return 0;
}

int dmvae::decode_hidden(dmvae_plan* p, hipStream_t s) {
    const PAct* in = &p->a.Z;
    for (size_t i = 0; i < p->dec.size(); ++i) {
        TRY(fwd_dense(p, s, *in, p->dec[i], DMVAE_EPI_BIAS_RELU, p->a.dec[i]));
        in = &p->a.dec[i];
    }
    return 0;
}

// The MoE stage of a pass, behind the latent stage (which has written logits, mean, gmu and dlogits): expert outputs P (a GEMM with the
// bias epilogue off the batch; featLearn: inside the row kernel), the row kernel (gate, mixture, loss, dP, dlogits / gmu terms), and the
// expert layer's weight-gradient problem (queued with the others on bf16 plans).
int dmvae::moe_stage(dmvae_plan* p, hipStream_t s, int n_valid, float inv_B, bool backward) {
    auto& M = p->moe;
    const dmvae_config& c = p->cfg;
    const bool fl = M.cfg.featLearn != 0;
    if (!fl) TRY(fwd_dense(p, s, XB(p), M.L, DMVAE_EPI_BIAS_F32, M.P));
    MoeHeadArgs a;
    memset(&a, 0, sizeof(a));
    a.B = n_valid; a.B_pad = p->Bp; a.E = M.cfg.n_experts; a.O = M.cfg.output_dim;
    a.featLearn = fl; a.classification = M.cfg.classification != 0; a.backward = backward; a.act_dtype = c.dtype;
    a.inv_B = inv_B;
    a.P = WSf(p, M.P); a.ldP = M.P.ld;
    a.logits = WSf(p, p->a.lg); a.ld_lg = p->a.lg.ld;
    a.Y = M.cfg.labels; a.n_rows = M.cfg.label_rows;
    a.perm = M.perm; a.first = M.first; a.batch = c.max_batch; a.st = reinterpret_cast<const dmvae_state*>(M.st);
    a.mean = WSf(p, p->a.mv); a.ld_mean = p->a.mv.ld; a.D = c.latent_dim; a.Dp = p->Dp;
    a.W = p->buf.param + M.L.w_off; a.ldW = M.L.ldw; a.bias = p->buf.param + M.L.b_off;
    a.inp_act = WS(p, M.inp); a.ld_inp = M.inp.ld;
    a.gmu = WSf(p, p->a.gmu); a.ld_g = p->a.gmu.ld;
    a.dP_act = WS(p, M.dP); a.ld_dP = M.dP.ld;
    a.dlogits_act = WS(p, p->a.dlg); a.ld_dl = p->a.dlg.ld;
    a.dq_ws = WSf(p, M.dq); a.ld_dq = M.dq.ld;
    a.pred = WSf(p, M.pred); a.ld_pred = M.pred.ld;
    a.partials = WSf(p, M.o_part);
    a.acc = WSf(p, M.acc);
    TRY(moe_head_launch(s, a));
    if (!backward) return 0;
    return grad_dense(p, s, fl ? M.inp : XB(p), M.dP, M.L);
}

// The label stage of a pass, behind the latent stage (which has written logits and dlogits): the cross-entropy on q(c|x) of the labelled rows
// added into dlogits before the heads' backward reads it (label_xent.hip).  One launch; the weight w is read on the device.
int dmvae::label_stage(dmvae_plan* p, hipStream_t s, int n_valid, float inv_B) {
    const auto& L = p->lab;
    LabelXentArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = WSf(p, p->a.lg); a.ld_lg = p->a.lg.ld;
    a.n_valid = n_valid; a.K = p->cfg.n_classes;
    a.labels = L.labels; a.label_rows = L.rows;
    a.perm = p->moe.perm; a.first = p->moe.first; a.batch = p->cfg.max_batch; a.st = reinterpret_cast<const dmvae_state*>(p->moe.st);
    a.act_dtype = p->cfg.dtype;
    a.scale = inv_B; a.w = WSf(p, L.o_ctl);
    a.dlogits = WS(p, p->a.dlg); a.ld_dl = p->a.dlg.ld;
    a.acc = reinterpret_cast<double*>(WS(p, L.o_acc));
    a.err_flag = reinterpret_cast<int32_t*>(WS(p, L.o_err));
    return label_xent_launch(s, a, "dmvae_plan_forward_backward (label stage)");
}

// ====================================================================== the pass
// What one forward + backward pass decides once, before its first launch.
struct Pass {
    hipStream_t s;
    int n_valid, stage;               // stage < 0: the whole pass
    bool all;
    float inv_B, vae_inv_B;           // vae_inv_B: the scale of the VAE terms' gradients
    bool hl_fused;                    // heads forward + latent stage as one launch (heads_latent.hip)
    bool heads_big;                   // the heads' dX GEMMs take the macro tile one by one instead of the grouped grid
    dmvae_finalize_args fin;          // step_finalize: a launch of its own, or riding ...
    bool fin_rides, fin_in_dz, fin_in_out;      // ... in the dZ GEMM / the output layer's dX launch / (neither) the heads' grouped dX launch
    GemmRiders rid_dz, rid_out;       // the riders of those two launches (step_finalize blocks, a prefetched batch's gather)
    dmvae_latent_args la;
};

// K slices of this pass's dW groups (dw_slices_max).  MEASURED (tools/knob_step.py <cfg> 10 1 2 4, same box):
// cfg3 (16384 rows) 1.0065 / 0.9778 / 0.9855 ms per step for 1 / 2 / 4 slices; cfg4 (8192 rows) 0.6623 / 0.7003 / 0.7126 -- the
// slabs' extra 8 B per parameter and the separate Adam pass pay only once a tile's K loop is > 128 K tiles: two slices from 16384 rows
// With the 256-divisible layers (three quarters of the flops of the MNIST-shaped stacks: [z|c]-hidden, 2048 -> 512, 512 -> 512)
// on the macro tile: four slices make 4 x 56 = 224 macro workgroups -- one round of the chip at 1.3-1.4 PFLOP/s against the
// small tiles' 0.74 in this layout (both operands through the transposing LDS read).
// MEASURED (same box, tools/knob_step.py <cfg> 11 0 1): cfg3 (16384 rows) 0.9565 (small tiles, two slices) -> 0.9388 ms per step
// (macro launch 98 us at 1.40 PFLOP/s + the small-tile remainder 120 us + the Adam pass 40 us); cfg4 (8192 rows) 0.6474
// (unsliced, fused Adam) vs 0.7248: a 2048-deep slice does not carry the slabs' extra pass -- from 16384 rows only.
static void pick_dw_slices(dmvae_plan* p) {
    const bool macro = g_dw_macro && p->dw_slices_max >= 4 && 4 * p->dw_macro_tiles >= 160 && p->Bp >= 16384 && gemm_bf16_256_slice_ok(256, 256, p->Bp / 4);
    const int want = g_dw_slices > 0 ? g_dw_slices : macro ? 4 : (p->Bp >= 16384 ? 2 : 1);
    p->dw_slices_now = (p->dw_slices_max > 1 && want > 1 && p->Bp % (want * 64) == 0) ? std::min(want, p->dw_slices_max) : 1;
    p->dw_macro_now = g_dw_macro && p->dw_slices_now > 1;
}

// the forms of the latent stage and of the heads' dX under the knobs' CURRENT values, and the step_finalize arguments
static int pick_forms(dmvae_plan* p, Pass& ps) {
    const dmvae_config& c = p->cfg;
    const int dt = c.dtype;
    // dmoe (lossVAE 0): the VAE terms scale their gradients by zero -- exact zeros for the decoder, the z-head and the prior tables,
    // whose Adam update then moves nothing (m = v = 0 stay 0); the reported VAE loss keeps inv_B
    ps.vae_inv_B = (p->moe.on && !p->moe.cfg.lossVAE) ? 0.f : ps.inv_B;
    // heads forward + latent stage as one launch where it applies (bf16, <= 4096 rows, Dp <= 128, K * D < 4096): blocks of 16 rows
    ps.hl_fused = dt == DMVAE_BF16 && !p->vade && heads_latent_ok(p->Bp, c.latent_dim, c.n_classes, p->Dp, p->Kp, p->Hp, c.mode, 16) && p->mv.ldw >= 2 * p->Dp && p->lg.ldw >= p->Kp;
    const int n_lblk = p->vade ? p->n_lblk : ps.hl_fused ? p->Bp / 16 : latent_nblocks(p->Bp, c.latent_dim, c.n_classes);      // under the knob's CURRENT value: what latent_launch will use
    const int n_pblk = p->lws_bytes ? 1 : n_lblk;
    DMVAE_REQUIRE(n_lblk <= p->n_lblk_cap, "dmvae_plan_forward_backward: the latent kernel would run %d blocks, the plan's partial-sum buffers hold %d", n_lblk, p->n_lblk_cap);
    ps.fin = step_finalize_args(WSf(p, p->o_rpart), p->n_rpart, WSf(p, p->o_lpart), n_lblk, ps.inv_B, p->buf.state, 1, c.beta1, c.beta2,
                                WSf(p, p->o_dprior), n_pblk, 2 * c.n_classes * c.latent_dim, p->buf.grad + p->prior_off);
    // (wide heads -- the 4096-wide configuration -- take the 256x256 macro-tile kernel one by one instead of the grouped grid)
    ps.heads_big = dt == DMVAE_BF16 && gemm_bf16_256_ok(DMVAE_GEMM_DX, DMVAE_EPI_RELU_MASK, p->Bp, p->Hp, 2 * p->Dp, false) &&
                   gemm_bf16_256_ok(DMVAE_GEMM_DX, DMVAE_EPI_RELU_MASK, p->Bp, p->Hp, p->Kp, false);
    return 0;
}

// Loss scalars, Adam t / lr_t and the prior-table gradients need only the forward partials.  Whole pass, bf16:
// the 1 + 80 blocks of step_finalize ride as extra workgroups of the grouped heads-dX launch further down (one
// kernel boundary less); staged (data parallel: the prior tables belong to this segment's bucket) and f32: a
// launch of their own (forward_and_loss).  MEASURED earlier: as a side BRANCH of the graph (fork / join events) the step
// took 0.344 ms against 0.326 ms -- a second branch costs more than the launch it hides.
static void place_riders(dmvae_plan* p, Pass& ps) {
    const dmvae_config& c = p->cfg;
    const int dt = c.dtype;
    ps.fin_rides = ps.all && dt == DMVAE_BF16 && !ps.heads_big && !p->vade && g_fin_rides;
    // ... and WHERE they ride.  In the heads' dX launch (every slot of the chip taken by a real workgroup) they cost that launch 2.2 us at 4096 rows
    // (MEASURED, knob 16: 19.4 us with them, 17.2 without; as a launch of their own +4.3 us per step).  The dZ GEMM two launches earlier has
    // their inputs too (it runs behind the reconstruction layer) and, while tiles + riders <= 256, leaves every rider a CU of its own.
    ps.fin_in_dz = ps.fin_in_out = false;
    const int fin_lead = (ps.fin.nblocks + 7) & ~7;
    GemmArgs dz_shape{}, out_shape{};           // (shapes only: what gemm_bf16_riders_room looks at)
    dz_shape.M = p->Bp; dz_shape.N = p->Dp; dz_shape.K = p->dec.empty() ? 64 : p->dec[0].out_pad; dz_shape.epi.kind = DMVAE_EPI_LATENT; dz_shape.k_split = dz_shape.K;
    out_shape.M = p->Bp; out_shape.N = p->dec.empty() ? 64 : p->dec.back().out_pad; out_shape.K = p->Ip; out_shape.epi.kind = DMVAE_EPI_RELU_MASK;
    const int dz_room = (dt == DMVAE_BF16 && !p->dec.empty()) ? gemm_bf16_riders_room(dz_shape, true) : -1;
    const int out_room = (dt == DMVAE_BF16 && !p->dec.empty()) ? gemm_bf16_riders_room(out_shape, false) : -1;
    // knob 16 = 3: step_finalize as second workgroups of the output layer's dX launch whenever it has the room (free there: 0.2717 vs 0.2721 ms
    // against the dZ placement) -- where it also goes by default when the dZ launch runs on its two-wave 16-row tiles, which cannot carry it
    if (ps.fin_rides && g_fin_rides == 3 && out_room >= fin_lead) ps.fin_in_out = true;
    if (ps.fin_rides && g_fin_rides == 1) ps.fin_in_dz = dz_room >= fin_lead && gemm_bf16_carries_finalize(dz_shape);
    if (ps.fin_rides && g_fin_rides == 1 && !ps.fin_in_dz && out_room >= fin_lead) ps.fin_in_out = true;      // (free there: 9.3 vs 9.2 us for that launch)
    // A prefetched batch (dmvae_plan_prefetch_batch): its gather takes the idle CUs of the dZ launch -- behind step_finalize, which has moved the
    // batch cursor on: those blocks then ride one launch EARLIER, as second workgroups of the output layer's dX launch (their inputs, the loss
    // partials, are complete behind the output layer's forward GEMM).  Without the room for both: step_finalize where it was, the gather as a
    // launch of its own in front of the trunk's backward pass.
    if (p->pf.armed && (ps.all || ps.stage == 0)) {
        p->pf.gat = gather_args(DMVAE_BF16, p->pf.data, p->pf.n_rows, c.input_dim, p->pf.perm, p->pf.first, c.max_batch, p->pf.n_valid, p->Bp, WS(p, XB(p, 1)), p->Ip,
                                nullptr, p->Ip, p->Ip, p->pf.st);
        if (ps.fin_rides && g_fin_rides == 1 && g_pf_rides && dz_room >= 64 && out_room >= fin_lead) {
            ps.fin_in_dz = false; ps.fin_in_out = true;
            ps.rid_dz.gat = p->pf.gat;
            ps.rid_dz.gat_last = g_pf_rides != 2;           // behind the tiles: the tiles then get CUs of their own first
            ps.rid_dz.ngat = (g_pf_rides == 3 ? std::min(2 * dz_room, 512) : std::min(dz_room, 256)) & ~7;
        }
    }
    if (ps.fin_in_dz) { ps.rid_dz.fin = ps.fin; ps.rid_dz.nfin = fin_lead; }
    if (ps.fin_in_out) { ps.rid_out.fin = ps.fin; ps.rid_out.nfin = fin_lead; }
}

static void latent_args_of(const dmvae_plan* p, Pass& ps, const float* eps, int64_t ld_eps, const float* gumbel, int64_t ld_gumbel) {
    const dmvae_config& c = p->cfg;
    const auto& a = p->a;
    dmvae_latent_args& la = ps.la;
    memset(&la, 0, sizeof(la));
    latent_inputs(p, la, eps, ld_eps);
    latent_sample(p, la);
    la.B = ps.n_valid; la.mode = p->vade ? 2 : c.mode; la.act_dtype = c.dtype;
    la.kl_ratio = 1.f; la.temperature = c.temperature; la.inv_B = ps.vae_inv_B; la.noise_step = 0;
    la.logits = WSf(p, a.lg); la.ld_logits = a.lg.ld;
    la.gumbel = gumbel; la.ld_gumbel = ld_gumbel;
    la.weights = WSf(p, a.w); la.ld_w = a.w.ld;
    la.gmu = WSf(p, a.gmu); la.glv = WSf(p, a.glv); la.clv = WSf(p, a.clv); la.ld_g = a.gmu.ld;
    la.dlogits_act = WS(p, a.dlg); la.ld_dl = a.dlg.ld;
    la.dprior_partials = WSf(p, p->o_dprior);
    la.loss_partials = WSf(p, p->o_lpart);
    la.state = p->buf.state;
    la.mfma_ws = p->lws_bytes ? WS(p, p->o_lws) : nullptr; la.mfma_ws_bytes = p->lws_bytes;
}

// the two head layers inside the latent launch (heads_latent.hip)
static int heads_latent_stage(dmvae_plan* p, const Pass& ps) {
    dmvae_heads_args ha;
    memset(&ha, 0, sizeof(ha));
    ha.hz = WS(p, p->a.hzc); ha.lda = p->a.hzc.ld; ha.Hp = p->Hp; ha.Dp = p->Dp; ha.Kp = p->Kp;
    ha.W_mv = Wp(p, p->mv.w_off); ha.ld_mv = p->mv.ldw; ha.W_lg = Wp(p, p->lg.w_off); ha.ld_lg = p->lg.ldw;
    ha.b_mv = p->buf.param + p->mv.b_off; ha.b_lg = p->buf.param + p->lg.b_off;
    // few blocks (a small batch): K slices, while blocks x slices stay within one round of the chip (the scheme of ksplit_for)
    if (g_ksplit && p->o_ksws >= 0) {
        int S = KSPLIT_MAX_SLICES;
        while (S > 1 && (p->Hp % (S * 64) || (p->Bp / 16) * S > 256 || heads_latent_kslice_floats(p->Bp, p->Dp, S) > p->ksws_elems)) S /= 2;
        if (S > 1) {
            ha.kslices = S; ha.kslice_ws = WSf(p, p->o_ksws); ha.kslice_ws_floats = p->ksws_elems;
            ha.kslice_tick = reinterpret_cast<int32_t*>(WS(p, p->o_ktick));
        }
    }
    return heads_latent_launch(ps.s, &ps.la, &ha);
}

// output layer + reconstruction loss + dLoss/dlogits in one epilogue
static int output_layer_recon(dmvae_plan* p, const Pass& ps) {
    const dmvae_config& c = p->cfg;
    const PLayer& L = p->out;
    const PAct& in = p->a.dec.back();
    const PAct& dl = p->a.dl;
    DMVAE_REQUIRE(in.cols == L.in_pad && dl.cols == L.out_pad, "output layer: views of %d -> %d columns on a %d -> %d layer", in.cols, dl.cols, L.in_pad, L.out_pad);
    dmvae_epilogue e;
    memset(&e, 0, sizeof(e));
    e.kind = DMVAE_EPI_BIAS_RECON; e.m_valid = ps.n_valid; e.n_valid = c.input_dim; e.recon_kind = c.input_type; e.scale = ps.vae_inv_B;
    e.out = WS(p, dl); e.ldo = dl.ld; e.bias = p->buf.param + L.b_off;
    e.aux0 = WS(p, p->a.xf); e.ld0 = p->a.xf.ld; e.partials = WSf(p, p->o_rpart);
    if (p->tsrc_valid) {      // dmvae_plan_load_batch_step: the targets come from the dataset through the permutation (gemm_bf16_body)
        e.recon_kind |= 0x100;
        e.aux0 = p->tsrc.data; e.ld0 = c.input_dim; e.aux1 = p->tsrc.perm; e.ld1 = p->tsrc.first;
        e.aux2 = p->tsrc.st; e.d_off = c.max_batch; e.ld2 = p->tsrc.n_rows;
        DMVAE_REQUIRE(p->tsrc.n_valid == ps.n_valid, "dmvae_plan_forward_backward: n_valid=%d, but dmvae_plan_load_batch_step assembled %d rows", ps.n_valid, p->tsrc.n_valid);
        DMVAE_REQUIRE(!p->tsrc_used, "dmvae_plan_forward_backward: the batch assembled by dmvae_plan_load_batch_step has been consumed by an earlier pass "
                                     "(it has no f32 copy and the batch cursor has advanced): load the batch again, or use dmvae_plan_load_batch");
        // (only a batch addressed by the DEVICE cursor goes stale: step_finalize advances the cursor.  With an explicit `first` the bf16
        //  batch and the targets are both addressed by it, and a second pass over the same batch -- gradient checks, repeat passes -- is valid)
        if (p->tsrc.st) p->tsrc_used = true;
    }
    const int dt = c.dtype;
    if (!(dt == DMVAE_BF16 && dl.cs >= 0 && gemm_bf16_256_ok(DMVAE_GEMM_FWD, DMVAE_EPI_BIAS_RECON, p->Bp, L.out_pad, L.in_pad, false)))
        return gemm_checked(ps.s, dt, DMVAE_GEMM_FWD, p->Bp, L.out_pad, L.in_pad, WS(p, in), in.ld, Wp(p, L.w_off), L.ldw, &e, 1);
    GemmArgs a;      // the macro-tile kernel also leaves dLoss/dlogits' column sums = the output bias gradient
    TRY(gemm_checked(ps.s, dt, DMVAE_GEMM_FWD, p->Bp, L.out_pad, L.in_pad, WS(p, in), in.ld, Wp(p, L.w_off), L.ldw, &e, 1, &a));
    a.csum_out = WSf(p, dl.cs); a.csum_ld = dl.ld;
    dl.mark_cs_live();
    return gemm_bf16_dispatch(ps.s, DMVAE_GEMM_FWD, a, 1);
}

static int forward_and_loss(dmvae_plan* p, Pass& ps) {
    auto& a = p->a;
    p->dw_queue.clear();
    a.dl.cs_live = a.dhzc.cs_live = false;      // no dY of this pass has its column sums yet
    for (auto& d : a.ddec) d.cs_live = false;
    for (auto& d : a.denc) d.cs_live = false;
    TRY(encode_impl(p, ps.s, !ps.hl_fused));
    if (ps.hl_fused) TRY(heads_latent_stage(p, ps));
    else TRY(latent_launch(ps.s, &ps.la));
    if (p->moe.on) TRY(moe_stage(p, ps.s, ps.n_valid, ps.inv_B, true));
    if (p->lab.on) TRY(label_stage(p, ps.s, ps.n_valid, ps.inv_B));
    TRY(decode_hidden(p, ps.s));
    TRY(output_layer_recon(p, ps));
    if (ps.fin_rides) return 0;
    const dmvae_finalize_args& f = ps.fin;
    return step_finalize_launch(ps.s, f.rp, f.nr, f.lp, f.nl, ps.inv_B, p->buf.state, 1, p->cfg.beta1, p->cfg.beta2, f.part, f.nblk, f.ncol, f.gout);
}

// dZ -> [dmean | dlog_var] through the reparameterisation + KL gradients; the step_finalize blocks, or the next batch's gather, may ride here (place_riders)
static int dz_gemm(dmvae_plan* p, Pass& ps) {
    const PLayer& L = p->dec[0];
    const PAct &dy = p->a.ddec[0], &dmv = p->a.dmv;
    const int dt = p->cfg.dtype;
    dmvae_epilogue e;
    memset(&e, 0, sizeof(e));
    e.kind = DMVAE_EPI_LATENT; e.out = WS(p, dmv); e.ldo = dmv.ld; e.d_off = p->Dp;
    e.aux0 = ps.la.gmu; e.ld0 = p->a.gmu.ld; e.aux1 = ps.la.glv; e.ld1 = p->a.glv.ld; e.aux2 = ps.la.clv; e.ld2 = p->a.clv.ld;
    const int S = ksplit_for(p, p->Dp, L.out_pad, DMVAE_EPI_LATENT);      // a small batch: K slices (GemmArgs::tick)
    const bool riders = ps.rid_dz.nfin || ps.rid_dz.ngat;
    if (!riders && S == 1) return gemm_checked(ps.s, dt, DMVAE_GEMM_DX, p->Bp, p->Dp, L.out_pad, WS(p, dy), dy.ld, Wp(p, L.w_off), L.ldw, &e, 1);
    GemmArgs ga;
    TRY(gemm_checked(ps.s, dt, DMVAE_GEMM_DX, p->Bp, p->Dp, L.out_pad, WS(p, dy), dy.ld, Wp(p, L.w_off), L.ldw, &e, 1, &ga));
    if (S > 1) kslice(p, ga, S);
    TRY(gemm_bf16_dispatch(ps.s, DMVAE_GEMM_DX, ga, S, riders ? &ps.rid_dz : nullptr));
    if (ps.rid_dz.ngat) { p->pf.armed = false; p->pf.done = true; }
    return 0;
}

static int backward_decoder(dmvae_plan* p, Pass& ps) {
    const auto& a = p->a;
    const int nd = (int)p->dec.size();
    TRY(grad_dense(p, ps.s, a.dec[nd - 1], a.dl, p->out));
    TRY(dx_dense(p, ps.s, a.dl, p->out, a.dec[nd - 1], a.ddec[nd - 1], nullptr, ps.fin_in_out ? &ps.rid_out : nullptr));
    for (int i = nd - 1; i >= 0; --i) {
        TRY(grad_dense(p, ps.s, i > 0 ? a.dec[i - 1] : a.Z, a.ddec[i], p->dec[i]));
        if (i > 0) TRY(dx_dense(p, ps.s, a.ddec[i], p->dec[i], a.dec[i - 1], a.ddec[i - 1]));
        else TRY(dz_gemm(p, ps));
    }
    return flush_dw(p, ps.s, 0);   // decoder dW group (launched here only when staged / DMVAE_DW_OVERLAP)
}

static int backward_heads(dmvae_plan* p, Pass& ps) {
    const auto& a = p->a;
    const int ne = (int)p->enc.size();
    if (p->vade) {      // VaDE's heads are the one linear layer [mean | log_var] off the trunk
        TRY(grad_dense(p, ps.s, a.enc[ne - 1], a.dmv, p->mv));
        TRY(dx_dense(p, ps.s, a.dmv, p->mv, a.enc[ne - 1], a.denc[ne - 1]));
        return flush_dw(p, ps.s, 1);
    }
    const PAct hz = a.hzc.sub(0, p->Hp), hc = a.hzc.sub(p->Hp, p->Hp);
    TRY(grad_dense(p, ps.s, hz, a.dmv, p->mv));
    TRY(grad_dense(p, ps.s, hc, a.dlg, p->lg));
    {   // d(z-hidden) and d(c-hidden): independent siblings writing the two halves of dhzc -> one grouped grid (bf16)
        GemmArgs q[2];
        const bool grp = p->cfg.dtype == DMVAE_BF16 && !ps.heads_big;
        const dmvae_finalize_args* fin = (ps.fin_rides && !ps.fin_in_dz && !ps.fin_in_out) ? &ps.fin : nullptr;
        TRY(dx_dense(p, ps.s, a.dmv, p->mv, hz, a.dhzc.sub(0, p->Hp), grp ? &q[0] : nullptr));
        TRY(dx_dense(p, ps.s, a.dlg, p->lg, hc, a.dhzc.sub(p->Hp, p->Hp), grp ? &q[1] : nullptr));
        if (grp && g_heads_dx_form == 2) {       // z-hidden as its own launch, c-hidden (and the riding finalize blocks) as a group of one
            TRY(gemm_bf16_dispatch(ps.s, DMVAE_GEMM_DX, q[0], 1));
            TRY(gemm_bf16_grouped(ps.s, DMVAE_GEMM_DX, q + 1, 1, fin));
        } else if (grp) TRY(gemm_bf16_grouped(ps.s, DMVAE_GEMM_DX, q, 2, fin));
    }
    TRY(grad_dense(p, ps.s, a.enc[ne - 1], a.dhzc, p->zc));      // (the trunk's last activation feeds the [z|c]-hidden layer)
    return flush_dw(p, ps.s, 1);      // heads dW group ([mean|log_var], logits, [zh|ch]): launched here when staged
}

static int backward_trunk(dmvae_plan* p, Pass& ps) {
    const auto& a = p->a;
    const int ne = (int)p->enc.size();
    // a prefetched batch that did not ride in the dZ launch: a gather of its own, here -- step_finalize has run (in every placement it has, an
    // earlier launch of this stream), so the device cursor is the next batch's
    if (p->pf.armed) {
        const dmvae_gather_args& g = p->pf.gat;
        TRY(gather_launch(ps.s, DMVAE_BF16, g.data, g.n_rows, g.dim, g.perm, g.first, g.batch, g.n_valid, g.B_pad, g.out_act, g.ld_act, nullptr, g.ld_f32, g.cols_pad, g.st));
        p->pf.armed = false; p->pf.done = true;
    }
    if (!p->vade) TRY(dx_dense(p, ps.s, a.dhzc, p->zc, a.enc[ne - 1], a.denc[ne - 1]));
    for (int i = ne - 1; i >= 0; --i) {
        TRY(grad_dense(p, ps.s, i > 0 ? a.enc[i - 1] : trunk_input(p), a.denc[i], p->enc[i]));
        if (i > 0) TRY(dx_dense(p, ps.s, a.denc[i], p->enc[i], a.enc[i - 1], a.denc[i - 1]));
        else if (!p->conv.empty()) TRY(dx_dense(p, ps.s, a.denc[0], p->enc[0], a.cflat, a.dflat));   // gradient of the flattened pool output (gate: pool output > 0, see conv_trunk_backward)
    }
    TRY(flush_dw(p, ps.s, 2));   // trunk dW group (everything queued so far when not staged)
    return p->conv.empty() ? 0 : conv_trunk_backward(p, ps.s);
}

// stage < 0: the whole forward + backward.  stage 0 / 1 / 2: the three segments after which one
// contiguous BUCKET of the gradient arena is complete (dmvae_plan_grad_buckets): 0 = forward, loss,
// decoder backward -> [dec0 .. out, prior tables]; 1 = heads -> [zh|ch, mean|log_var, logits];
// 2 = trunk -> [enc*].  Each segment launches its own dW group, so a data-parallel caller can start
// the bucket's all-reduce while the next segment runs.
static int forward_backward_impl(dmvae_plan* p, void* stream, int n_valid, const float* eps, int64_t ld_eps,
                                 const float* gumbel, int64_t ld_gumbel, float inv_B, int stage) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_forward_backward: plan not bound");
    DMVAE_REQUIRE(n_valid > 0 && n_valid <= p->cfg.max_batch, "dmvae_plan_forward_backward: n_valid=%d out of range", n_valid);
    DMVAE_REQUIRE(stage >= -1 && stage <= 2, "dmvae_plan_forward_backward_stage: stage %d (0, 1, 2)", stage);
    if (p->moe.on && stage >= 0) { set_error("dmvae_plan_forward_backward_stage: not with a MoE attachment (one rank)"); return DMVAE_EUNSUPPORTED; }
    Pass ps;
    ps.s = (hipStream_t)stream; ps.n_valid = n_valid; ps.stage = stage; ps.all = stage < 0; ps.inv_B = inv_B;
    p->staged = !ps.all;
    if (ps.all || stage == 0) pick_dw_slices(p);
    TRY(pick_forms(p, ps));
    place_riders(p, ps);
    latent_args_of(p, ps, eps, ld_eps, gumbel, ld_gumbel);
    if (ps.all || stage == 0) {
        TRY(forward_and_loss(p, ps));
        TRY(backward_decoder(p, ps));
    }
    if (ps.all || stage == 1) TRY(backward_heads(p, ps));
    if (ps.all || stage == 2) TRY(backward_trunk(p, ps));
    return 0;
}

extern "C" int dmvae_plan_forward_backward(dmvae_plan* p, void* stream, int n_valid, const float* eps, int64_t ld_eps,
                                           const float* gumbel, int64_t ld_gumbel, float inv_B) {
    return forward_backward_impl(p, stream, n_valid, eps, ld_eps, gumbel, ld_gumbel, inv_B, -1);
}
extern "C" int dmvae_plan_forward_backward_stage(dmvae_plan* p, void* stream, int stage, int n_valid, const float* eps, int64_t ld_eps,
                                                 const float* gumbel, int64_t ld_gumbel, float inv_B) {
    DMVAE_REQUIRE(stage >= 0 && stage <= 2, "dmvae_plan_forward_backward_stage: stage %d (0, 1, 2)", stage);
    return forward_backward_impl(p, stream, n_valid, eps, ld_eps, gumbel, ld_gumbel, inv_B, stage);
}

extern "C" int dmvae_plan_train_step(dmvae_plan* p, void* stream, int n_valid, const float* eps, int64_t ld_eps,
                                     const float* gumbel, int64_t ld_gumbel, float inv_B) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_train_step: plan not bound");
    if (p->cfg.dtype != DMVAE_BF16 || !p->conv.empty()) {     // f32, or conv gradients (not in the dW group): the plain pair
        TRY(dmvae_plan_forward_backward(p, stream, n_valid, eps, ld_eps, gumbel, ld_gumbel, inv_B));
        return dmvae_plan_update(p, stream, 1.f);
    }
    p->fused_update = true;               // dW problems are queued with DMVAE_EPI_ADAM; flush_dw launches them with the Adam context
    const int rc = dmvae_plan_forward_backward(p, stream, n_valid, eps, ld_eps, gumbel, ld_gumbel, inv_B);
    p->fused_update = false;
    return rc;
}

extern "C" int dmvae_plan_update(dmvae_plan* p, void* stream, float grad_scale) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_update: plan not bound");
    return dmvae_plan_update_range(p, stream, grad_scale, 0, p->param_elems);
}
extern "C" int dmvae_plan_update_range(dmvae_plan* p, void* stream, float grad_scale, int64_t lo, int64_t hi) {
    DMVAE_REQUIRE(p && p->bound, "dmvae_plan_update_range: plan not bound");
    DMVAE_REQUIRE(lo >= 0 && hi > lo && hi <= p->buf.arena_elems && lo % 4 == 0 && hi % 4 == 0,
                  "dmvae_plan_update_range: [%lld, %lld) must be a 4-aligned range of the %lld-element arena", (long long)lo, (long long)hi, (long long)p->buf.arena_elems);
    AdamArgs a;
    a.n = hi - lo; a.p = p->buf.param + lo; a.g = p->buf.grad + lo; a.m = p->buf.m + lo; a.v = p->buf.v + lo;
    a.pb = p->cfg.dtype == DMVAE_BF16 ? reinterpret_cast<bf16_t*>(p->buf.param_bf16) + lo : nullptr;
    a.lr = 0.f; a.b1 = p->cfg.beta1; a.b2 = p->cfg.beta2; a.eps = p->cfg.adam_eps; a.gscale = grad_scale;
    a.zero_grad = 0;    // every gradient element is overwritten each step (no atomic accumulation)
    a.ieee = p->cfg.adam_ieee;
    a.t_host = ~0ull;    // t = state->adam_t, already advanced by this step's loss_finalize (saves a launch)
    a.st = reinterpret_cast<const dmvae_state*>(p->buf.state);
    return adam_launch((hipStream_t)stream, a);
}
