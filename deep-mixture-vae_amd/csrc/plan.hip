// The step plan (plan.h): arena layout, workspace layout -- the one place that states a buffer's shape --, binding, the MoE attachment, views.
#include <stdlib.h>

#include <algorithm>

#include "plan.h"
#include "moe_head.h"
#include "label_xent.h"

using namespace dmvae;

static inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
// the next bytes of the workspace (256-byte granules); a [rows][cols] activation of es-byte elements
static int64_t take(int64_t& w, int64_t bytes) { int64_t o = w; w += align_up(bytes, 256); return o; }
static PAct take_act(int64_t& w, int64_t rows, int cols, int es) {
    PAct a;
    a.off = take(w, rows * cols * es); a.cols = cols; a.ld = cols; a.es = es;
    return a;
}

static void add_tensor(dmvae_plan* p, const std::string& name, int64_t off, int rows, int cols, int64_t ld) {
    dmvae_tensor_info t;
    memset(&t, 0, sizeof(t));
    snprintf(t.name, sizeof(t.name), "%s", name.c_str());
    t.offset = off; t.rows = rows; t.cols = cols; t.ld = ld;
    p->tensors.push_back(t);
}

extern "C" int dmvae_plan_create(const dmvae_config* c, dmvae_plan** out) {
    DMVAE_REQUIRE(c && out, "dmvae_plan_create: null argument");
    DMVAE_REQUIRE(c->input_dim > 0 && c->latent_dim > 0 && c->n_classes > 0 && (c->head_dim > 0 || c->model == DMVAE_MODEL_VADE), "dmvae_plan_create: bad dims");
    DMVAE_REQUIRE(c->model == DMVAE_MODEL_DMVAE || (c->model == DMVAE_MODEL_VADE && c->mode == 0),
                  "dmvae_plan_create: model %d (0 DMVAE, 1 VaDE; VaDE runs the exact KL)", c->model);
    DMVAE_REQUIRE(c->n_enc >= 1 && c->n_enc <= DMVAE_MAX_LAYERS && c->n_dec >= 1 && c->n_dec <= DMVAE_MAX_LAYERS, "dmvae_plan_create: 1..%d layers", DMVAE_MAX_LAYERS);
    DMVAE_REQUIRE(c->dtype == DMVAE_F32 || c->dtype == DMVAE_BF16, "dmvae_plan_create: bad dtype");
    DMVAE_REQUIRE(c->max_batch > 0, "dmvae_plan_create: max_batch must be > 0");
    dmvae_plan* p = new dmvae_plan();
    p->cfg = *c;
    p->bound = false;
    p->es = c->dtype == DMVAE_BF16 ? 2 : 4;
    p->Bp = (c->max_batch + 127) / 128 * 128;
    p->Ip = pad64(c->input_dim);
    p->Dp = pad64(c->latent_dim);
    p->Kp = pad64(c->n_classes);
    p->vade = c->model == DMVAE_MODEL_VADE;
    p->Hp = pad64(p->vade ? 64 : c->head_dim);
    // Arena layout: every weight matrix first (trunk, heads, decoder, output), then -- from tail_off, a multiple of 4096 elements --
    // the SMALL fp32 tensors: every bias in the same layer order, then the prior tables.  The GEMMs read the weights through the bf16
    // shadow; the biases (epilogues) and the prior tables (latent kernel) are read in fp32.  Kept apart, a data-parallel job can
    // reduce-scatter / shard-update the weight range and all-gather its bf16 SHADOW (half the bytes) while the tail
    // is all-reduced whole and updated on every rank (dmvae_plan_grad_buckets).  boff counts tail-relative until tail_off is known.
    int64_t off = 0, boff = 0;
    auto place = [&](PLayer& L, const std::string& name, int in, int out_, int in_pad, int out_pad) {
        L.name = name; L.in = in; L.out = out_; L.in_pad = in_pad; L.out_pad = out_pad; L.ldw = out_pad;
        L.w_off = off; off += (int64_t)in_pad * out_pad;
        L.b_off = boff; boff += out_pad;
    };
    int prev = c->input_dim, prev_pad = p->Ip;
    if (c->trunk == DMVAE_TRUNK_CNN) {
        // the checked-in encoder (base_models.py:176-216): reshape (-1,28,28,1); conv 1-32, 32-32, pool, 32-64, 64-64,
        // pool, 64-128, 128-128, pool (SAME: 28 -> 14 -> 7 -> 4); flatten (h,w,c) = 2048; FullyConnected 2048 -> enc[0]
        if (c->input_dim != 784 || c->n_enc != 1) { delete p; set_error("dmvae_plan_create: the CNN trunk takes 784 inputs and one fc layer"); return DMVAE_EINVAL; }
        static const int spec[6][4] = {{1, 32, 28, 0}, {32, 32, 28, 1}, {32, 64, 14, 0}, {64, 64, 14, 1}, {64, 128, 7, 0}, {128, 128, 7, 1}};
        int ld_in = 1;
        for (int i = 0; i < 6; ++i) {
            PConv L;
            L.name = "conv" + std::to_string(i);
            L.cin = spec[i][0]; L.cout = spec[i][1]; L.hw = spec[i][2]; L.pool = spec[i][3];
            L.cin_ld = ld_in; L.cout_ld = L.cout; L.cin_np = pad64(L.cin); L.cout_np = pad64(L.cout); L.P = L.hw + 2;
            L.kdim = pad64(9 * L.cin); L.ktdim = pad64(9 * L.cout);
            L.w_off = off; off += (int64_t)L.kdim * L.cout_np;
            L.b_off = boff; boff += L.cout_np;
            add_tensor(p, "W_" + L.name, L.w_off, 9 * L.cin, L.cout, L.cout_np);
            add_tensor(p, "b_" + L.name, L.b_off, 1, L.cout, L.cout_np);
            p->conv.push_back(L);
            ld_in = L.cout_ld;
        }
        p->conv_param_end = off;
        p->flat = 4 * 4 * 128;
        prev = p->flat; prev_pad = p->flat;
    }
    auto stack = [&](std::vector<PLayer>& v, const char* tag, int n, const int* widths) {
        for (int i = 0; i < n; ++i) {
            PLayer L;
            place(L, tag + std::to_string(i), prev, widths[i], prev_pad, pad64(widths[i]));
            add_tensor(p, "W_" + L.name, L.w_off, L.in, L.out, L.ldw);
            add_tensor(p, "b_" + L.name, L.b_off, 1, L.out, L.out_pad);
            v.push_back(L);
            prev = widths[i]; prev_pad = L.out_pad;
        }
    };
    stack(p->enc, "enc", c->n_enc, c->enc);
    p->Tp = prev_pad;
    if (!p->vade) {
        place(p->zc, "zc", prev, 2 * p->Hp, p->Tp, 2 * p->Hp);
        add_tensor(p, "W_zh", p->zc.w_off, prev, c->head_dim, p->zc.ldw);
        add_tensor(p, "b_zh", p->zc.b_off, 1, c->head_dim, 2 * p->Hp);
        add_tensor(p, "W_ch", p->zc.w_off + p->Hp, prev, c->head_dim, p->zc.ldw);
        add_tensor(p, "b_ch", p->zc.b_off + p->Hp, 1, c->head_dim, 2 * p->Hp);
    }
    // [mean | log_var]: off the z-hidden layer (DMVAE, base_models.py:234-239) or straight off the trunk (VaDE, :501-507)
    const int mv_in = p->vade ? prev : c->head_dim, mv_in_pad = p->vade ? p->Tp : p->Hp;
    place(p->mv, "mv", mv_in, 2 * p->Dp, mv_in_pad, 2 * p->Dp);
    add_tensor(p, "W_mean", p->mv.w_off, mv_in, c->latent_dim, p->mv.ldw);
    add_tensor(p, "b_mean", p->mv.b_off, 1, c->latent_dim, 2 * p->Dp);
    add_tensor(p, "W_logvar", p->mv.w_off + p->Dp, mv_in, c->latent_dim, p->mv.ldw);
    add_tensor(p, "b_logvar", p->mv.b_off + p->Dp, 1, c->latent_dim, 2 * p->Dp);
    if (!p->vade) {
        place(p->lg, "logits", c->head_dim, c->n_classes, p->Hp, p->Kp);
        add_tensor(p, "W_logits", p->lg.w_off, c->head_dim, c->n_classes, p->lg.ldw);
        add_tensor(p, "b_logits", p->lg.b_off, 1, c->n_classes, p->Kp);
    }
    prev = c->latent_dim; prev_pad = p->Dp;
    stack(p->dec, "dec", c->n_dec, c->dec);
    place(p->out, "out", prev, c->input_dim, prev_pad, p->Ip);
    add_tensor(p, "W_out", p->out.w_off, prev, c->input_dim, p->out.ldw);
    add_tensor(p, "b_out", p->out.b_off, 1, c->input_dim, p->Ip);
    p->tail_off = align_up(off, 4096);
    for (auto& L : p->conv) L.b_off += p->tail_off;
    for (auto& L : p->enc) L.b_off += p->tail_off;
    for (auto& L : p->dec) L.b_off += p->tail_off;
    p->zc.b_off += p->tail_off; p->mv.b_off += p->tail_off; p->lg.b_off += p->tail_off; p->out.b_off += p->tail_off;
    for (auto& t : p->tensors)
        if (t.name[0] == 'b' && t.name[1] == '_') t.offset += p->tail_off;
    off = p->tail_off + boff;
    p->prior_off = off;
    const int KD = c->n_classes * c->latent_dim;
    add_tensor(p, "prior_means", off, c->n_classes, c->latent_dim, c->latent_dim);
    add_tensor(p, "prior_log_vars", off + KD, c->n_classes, c->latent_dim, c->latent_dim);
    off += align_up(2 * (int64_t)KD, 64);
    p->param_elems = off;

    // ---- workspace: the order and the sizes of the take()s ARE the layout (tests/golden/plan_layout.json)
    int64_t w = 0;
    const int64_t Bp = p->Bp;
    const int es = p->es;
    auto& a = p->a;
    auto act = [&](int cols, int esz) { return take_act(w, Bp, cols, esz); };
    a.xf = act(p->Ip, 4);
    a.x = (c->dtype == DMVAE_F32) ? a.xf : act(p->Ip, es);
    if (c->dtype == DMVAE_BF16 && p->conv.empty()) a.x2 = act(p->Ip, es);
    if (!p->conv.empty()) {
        int64_t wmax = 0;
        for (size_t i = 0; i < p->conv.size(); ++i) {
            PConv& L = p->conv[i];
            auto bordered = [&](int P, int ld) { return take(w, (Bp * P * P + 2 * (P + 1)) * ld * es); };
            L.o_act = bordered(L.P, L.cout_ld);
            L.o_dact = bordered(L.P, L.cout_ld);
            const int ho = (L.hw + 1) / 2;
            const bool last = i + 1 == p->conv.size();
            L.o_pool = L.pool ? (last ? take(w, Bp * ho * ho * L.cout_ld * es) : bordered(ho + 2, L.cout_ld)) : 0;
            L.o_dpool = (L.pool && !last) ? bordered(ho + 2, L.cout_ld) : 0;
            if (i > 0) wmax = std::max<int64_t>(wmax, (int64_t)L.cin_np * L.ktdim);
        }
        a.cflat.off = p->conv.back().o_pool; a.cflat.cols = p->flat; a.cflat.ld = p->flat; a.cflat.es = es;      // (the last layer's plain pool output)
        p->o_wt = take(w, wmax * es);
        a.dflat = act(p->flat, es);
        p->o_c0part = take(w, (int64_t)conv_first_dw_blocks(p->conv.front().hw, Bp) * 320 * 4);
        // split-K slabs instead of float atomics (always: measured FASTER than the atomic form, 3.06 vs 3.23 ms/step): the largest layer's split x (kdim + 1) x cout_np floats
        int64_t mx = 0;
        for (size_t i = 1; i < p->conv.size(); ++i) {
            const PConv& L = p->conv[i];
            const int sp = conv_dw_split((int64_t)Bp * L.P * L.P, (L.kdim / 64) * (L.cout_np / 64));
            mx = std::max<int64_t>(mx, (int64_t)sp * (L.kdim + 1) * L.cout_np);
        }
        p->o_cslab = take(w, mx * 4);
    }
    for (auto& L : p->enc) a.enc.push_back(act(L.out_pad, es));
    a.hzc = act(2 * p->Hp, es);
    a.mv = act(2 * p->Dp, 4);
    a.lg = act(p->Kp, 4);
    a.Z = act(p->Dp, es);
    a.Zf = act(p->Dp, 4);
    a.gmu = act(p->Dp, 4);
    a.glv = act(p->Dp, 4);
    a.clv = act(p->Dp, 4);
    a.w = act(p->Kp, 4);
    a.dlg = act(p->Kp, es);
    for (auto& L : p->dec) a.dec.push_back(act(L.out_pad, es));
    a.recon = act(p->Ip, 4);
    a.dl = act(p->Ip, es);
    for (auto& L : p->dec) a.ddec.push_back(act(L.out_pad, es));
    a.dmv = act(2 * p->Dp, es);
    a.dhzc = act(2 * p->Hp, es);
    for (auto& L : p->enc) a.denc.push_back(act(L.out_pad, es));
    if (c->dtype == DMVAE_BF16 && p->Bp % 256 == 0 && !getenv("DMVAE_NO_CSUM")) {      // column-sum partials of every dY (PAct::cs)
        const int64_t tr = p->Bp / 256;
        a.dl.cs = take(w, tr * a.dl.ld * 4);
        a.dhzc.cs = take(w, tr * a.dhzc.ld * 4);
        for (auto& d : a.ddec) d.cs = take(w, tr * d.ld * 4);
        for (auto& d : a.denc) d.cs = take(w, tr * d.ld * 4);
    }
    p->n_rpart = gemm_partials(c->dtype, p->Bp, p->Ip);
    p->o_rpart = take(w, (int64_t)p->n_rpart * 4);
    p->n_lblk = p->vade ? latent_vade_nblocks(p->Bp) : latent_nblocks(p->Bp, c->latent_dim, c->n_classes);
    // The block count of the latent kernel follows a tuning knob (14) that may change after the plan exists: the partial-sum buffers are
    // sized for the LARGEST count any setting can produce (16 rows per block), the count in use is taken at enqueue time
    // (latent_blocks_now) and checked against this capacity.
    p->n_lblk_cap = std::max(p->n_lblk, (p->Bp + 15) / 16);
    p->o_lpart = take(w, (int64_t)p->n_lblk_cap * 2 * 4);
    // (VaDE: tables past the one-kernel form's LDS take latent_vade_mfma.hip -- the step and dmvae_plan_eval_clusters share this scratch)
    p->lws_bytes = p->vade ? (latent_vade_mfma_needed(c->latent_dim, c->n_classes) ? latent_vade_mfma_ws_bytes(p->Bp, c->latent_dim, c->n_classes, nullptr) : 0)
                 : latent_mfma_applies(c->latent_dim, c->n_classes, c->mode) ? latent_mfma_ws_bytes(p->Bp, c->latent_dim, c->n_classes) : 0;
    p->n_pblk = p->lws_bytes ? 1 : p->n_lblk;          // the MFMA form delivers the prior-table gradient complete, in one row
    p->o_dprior = take(w, (int64_t)(p->lws_bytes ? 1 : p->n_lblk_cap) * 2 * KD * 4);
    if (p->lws_bytes) p->o_lws = take(w, p->lws_bytes);
    if (c->dtype == DMVAE_BF16 && p->Bp <= 2048) {
        // dense launches (<= KSPLIT_MAX_ROWS rows; the largest user: a 512-wide output, 8 slices, 64 x 64 tiles) and the fused heads + latent launch
        // (blocks x slices <= 256: up to 2048 rows)
        int64_t need = p->Bp <= KSPLIT_MAX_ROWS ? (int64_t)(p->Bp / 64) * 8 * KSPLIT_MAX_SLICES * 4096 : 0;
        if (p->Dp == 64 || p->Dp == 128)
            for (int S = 2; S <= KSPLIT_MAX_SLICES; S *= 2)
                if ((p->Bp / 16) * S <= 256) need = std::max(need, heads_latent_kslice_floats(p->Bp, p->Dp, S));
        if (need > 0) {
            p->ksws_elems = need;
            p->o_ksws = take(w, p->ksws_elems * 4);
            p->o_ktick = take(w, 256 * 4);
        }
    }
    int maxN = std::max(std::max(2 * p->Hp, p->Ip), p->flat);
    for (auto& L : p->enc) maxN = std::max(maxN, L.out_pad);
    for (auto& L : p->dec) maxN = std::max(maxN, L.out_pad);
    maxN = std::max(maxN, 2 * KD);
    p->cs_elems = (int64_t)64 * maxN;
    p->o_cs = take(w, p->cs_elems * 4);
    {   // K slices of the dW group (see dw_slices_max): bf16, dense trunk, a batch of >= 8192 rows, no layer on the macro tile
        // every layer's problem + a bias strip for each layer the macro tile may take must fit ONE grouped launch queue: the fused
        // step sums the slabs once, behind it
        bool macro = false;
        int n_dw = 0, n_elig = 0, tiles = 0;
        auto cnt = [&](const PLayer& L) {
            macro = macro || gemm_bf16_256_ok(DMVAE_GEMM_DW, DMVAE_EPI_ADAM, L.in_pad, L.out_pad, (int)Bp, false);
            ++n_dw;
            if (L.in_pad % 256 == 0 && L.out_pad % 256 == 0) { ++n_elig; tiles += (L.in_pad / 256) * (L.out_pad / 256); }
        };
        for (auto& L : p->enc) cnt(L);
        for (auto& L : p->dec) cnt(L);
        if (!p->vade) { cnt(p->zc); cnt(p->lg); }
        cnt(p->mv); cnt(p->out);
        if (c->dtype == DMVAE_BF16 && p->conv.empty() && Bp >= 8192 && Bp % (4 * 64) == 0 && !macro && n_dw + n_elig < DMVAE_MAX_GROUP) {
            p->dw_slices_max = 4;
            p->o_dwslab = take(w, (int64_t)p->dw_slices_max * p->param_elems * 4);
            p->dw_macro_tiles = tiles;
        }
    }
    // the step path may leave the batch's f32 copy out (dmvae_plan_load_batch_step): bf16, 16-byte aligned dataset rows, and an
    // output layer that the small-tile kernel runs (the macro tile fetches its targets in row batches from the copy)
    p->tgt_gather = c->dtype == DMVAE_BF16 && c->input_dim % 4 == 0 &&
                    !gemm_bf16_256_ok(DMVAE_GEMM_FWD, DMVAE_EPI_BIAS_RECON, p->Bp, p->Ip, p->dec.back().out_pad, false);
    p->work_bytes = w;
    *out = p;
    return 0;
}

extern "C" void dmvae_plan_destroy(dmvae_plan* p) { delete p; }

extern "C" int dmvae_plan_sizes(const dmvae_plan* p, dmvae_sizes* o) {
    DMVAE_REQUIRE(p && o, "dmvae_plan_sizes: null argument");
    o->param_elems = p->param_elems;
    o->work_bytes = p->work_bytes;
    o->batch_pad = p->Bp;
    o->input_pad = p->Ip;
    o->n_tensors = (int)p->tensors.size();
    o->reserved = 0;
    return 0;
}
extern "C" int dmvae_plan_tensor(const dmvae_plan* p, int i, dmvae_tensor_info* o) {
    DMVAE_REQUIRE(p && o && i >= 0 && i < (int)p->tensors.size(), "dmvae_plan_tensor: bad index %d", i);
    *o = p->tensors[i];
    return 0;
}
extern "C" int dmvae_plan_bind(dmvae_plan* p, const dmvae_buffers* b) {
    DMVAE_REQUIRE(p && b && b->param && b->grad && b->m && b->v && b->work && b->state, "dmvae_plan_bind: null buffer");
    DMVAE_REQUIRE(p->cfg.dtype == DMVAE_F32 || b->param_bf16, "dmvae_plan_bind: bf16 plan needs the bf16 parameter shadow");
    DMVAE_REQUIRE((uintptr_t)b->work % 256 == 0 && (uintptr_t)b->param % 256 == 0 && (uintptr_t)b->grad % 256 == 0, "dmvae_plan_bind: buffers must be 256-byte aligned");
    p->buf = *b;
    if (p->buf.arena_elems == 0) p->buf.arena_elems = p->param_elems;
    DMVAE_REQUIRE(p->buf.arena_elems >= p->param_elems && p->buf.arena_elems % 4 == 0, "dmvae_plan_bind: arena_elems %lld < the plan's %lld parameters (or not a multiple of 4)",
                  (long long)p->buf.arena_elems, (long long)p->param_elems);
    p->bound = true;
    return 0;
}

// Mixture-of-experts attachment (models.py:10-163 of the reference).  W_moe goes behind the last weight matrix, the tail (every bias, then
// the prior tables) moves up behind it, b_moe is appended to the biases; the workspace grows by the MoE buffers.
extern "C" int dmvae_plan_attach_moe(dmvae_plan* p, const dmvae_moe_config* m) {
    DMVAE_REQUIRE(p && m, "dmvae_plan_attach_moe: null argument");
    DMVAE_REQUIRE(!p->bound && !p->moe.on, "dmvae_plan_attach_moe: attach once, before dmvae_plan_bind");
    if (p->lab.on) { set_error("dmvae_plan_attach_moe: not on a plan with a label attachment (dmvae_plan_attach_labels)"); return DMVAE_EUNSUPPORTED; }
    if (p->vade || !p->conv.empty() || p->dw_slices_max > 1) {
        set_error("dmvae_plan_attach_moe: the MoE head runs on DMVAE plans with the MLP trunk and fewer than 8192 rows (VaDE: its gate p(c|z) "
                  "sends gradients through Z; conv trunk: the flat input is not resident; larger batches: dW K-slices)");
        return DMVAE_EUNSUPPORTED;
    }
    const int E = m->n_experts, O = m->output_dim;
    DMVAE_REQUIRE(E == p->cfg.n_classes, "dmvae_plan_attach_moe: n_experts %d must equal the gate's n_classes %d", E, p->cfg.n_classes);
    DMVAE_REQUIRE(E >= 1 && E <= 256 && O >= 1 && O <= 64 && E * O <= 1024, "dmvae_plan_attach_moe: E=%d, O=%d (E <= 256, O <= 64, E*O <= 1024)", E, O);
    DMVAE_REQUIRE(m->labels && m->label_rows > 0, "dmvae_plan_attach_moe: null labels");
    auto& M = p->moe;
    M.cfg = *m;
    M.EO = E * O; M.EOp = pad64(M.EO);
    const bool fl = m->featLearn != 0;
    PLayer& L = M.L;
    L.name = "moe"; L.in = fl ? p->cfg.latent_dim : p->cfg.input_dim; L.in_pad = fl ? p->Dp : p->Ip; L.out = M.EO; L.out_pad = M.EOp; L.ldw = M.EOp;
    L.w_off = p->out.w_off + (int64_t)p->out.in_pad * p->out.out_pad;
    const int64_t tail = align_up(L.w_off + (int64_t)L.in_pad * L.ldw, 4096);
    const int64_t dt = tail - p->tail_off;                 // every tail tensor moves up by dt; the prior tables by dt + EOp more
    for (auto& c : p->conv) c.b_off += dt;
    for (auto& l : p->enc) l.b_off += dt;
    for (auto& l : p->dec) l.b_off += dt;
    p->zc.b_off += dt; p->mv.b_off += dt; p->lg.b_off += dt; p->out.b_off += dt;
    L.b_off = p->prior_off + dt;
    for (auto& t : p->tensors) {
        if (t.name[0] == 'b' && t.name[1] == '_') t.offset += dt;
        else if (!strncmp(t.name, "prior_", 6)) t.offset += dt + M.EOp;
    }
    p->tail_off = tail;
    p->prior_off += dt + M.EOp;
    p->param_elems += dt + M.EOp;
    add_tensor(p, "W_moe", L.w_off, L.in, M.EO, L.ldw);
    add_tensor(p, "b_moe", L.b_off, 1, M.EO, M.EOp);
    int64_t w = p->work_bytes;
    M.P = take_act(w, p->Bp, M.EOp, 4);
    M.dP = take_act(w, p->Bp, M.EOp, p->es);
    M.inp = take_act(w, p->Bp, p->Dp, p->es);
    M.dq = take_act(w, p->Bp, 256, 4);
    M.pred = take_act(w, p->Bp, 64, 4);
    M.nblk = moe_head_nblocks(p->Bp);
    M.o_part = take(w, (int64_t)M.nblk * 2 * 4);
    M.acc = take_act(w, 1, 4, 4);               // (one 256-byte granule: four floats)
    p->cs_elems = std::max<int64_t>(p->cs_elems, (int64_t)64 * M.EOp);
    p->o_cs = take(w, p->cs_elems * 4);        // (the column-sum scratch, grown if the expert layer is the widest)
    p->work_bytes = w;
    M.on = true;
    return 0;
}

extern "C" int dmvae_plan_moe_set_labels(dmvae_plan* p, const float* labels, int64_t label_rows) {
    DMVAE_REQUIRE(p && p->moe.on && labels && label_rows > 0, "dmvae_plan_moe_set_labels: no MoE attachment / null labels");
    p->moe.cfg.labels = labels; p->moe.cfg.label_rows = label_rows;
    return 0;
}

// Semi-supervised label attachment (label_xent.hip): no parameter, no GEMM problem -- the workspace grows by the control word, the
// accumulators (with the stage's partials, sized for the padded batch) and the error flag.
extern "C" int dmvae_plan_attach_labels(dmvae_plan* p, const dmvae_label_config* m) {
    DMVAE_REQUIRE(p && m, "dmvae_plan_attach_labels: null argument");
    DMVAE_REQUIRE(!p->bound && !p->lab.on, "dmvae_plan_attach_labels: attach once, before dmvae_plan_bind");
    if (p->vade) {
        set_error("dmvae_plan_attach_labels: not on a VaDE plan (its q(c|x) is p(c|z): the gradient would run through Z into the VaDE latent stage)");
        return DMVAE_EUNSUPPORTED;
    }
    if (p->moe.on) {
        set_error("dmvae_plan_attach_labels: not on a plan with a MoE attachment (its loss already owns the gate's labels)");
        return DMVAE_EUNSUPPORTED;
    }
    DMVAE_REQUIRE(m->labels && m->label_rows > 0 && m->reserved == 0, "dmvae_plan_attach_labels: null labels / label_rows=%lld / reserved != 0", (long long)m->label_rows);
    auto& L = p->lab;
    L.labels = m->labels; L.rows = m->label_rows;
    int64_t w = p->work_bytes;
    L.o_ctl = take(w, 256);
    L.acc_elems = label_xent_acc_elems(p->Bp);
    L.o_acc = take(w, L.acc_elems * 8);
    L.o_err = take(w, 256);
    p->work_bytes = w;
    L.on = true;
    return 0;
}

extern "C" int dmvae_plan_set_labels(dmvae_plan* p, const int32_t* labels, int64_t label_rows) {
    DMVAE_REQUIRE(p && p->lab.on && labels && label_rows > 0, "dmvae_plan_set_labels: no label attachment / null labels");
    p->lab.labels = labels; p->lab.rows = label_rows;
    return 0;
}

extern "C" int dmvae_plan_set_stage_groups(dmvae_plan* p, int n_groups) {
    DMVAE_REQUIRE(p && (n_groups == 2 || n_groups == 3), "dmvae_plan_set_stage_groups: 2 or 3 weight-gradient launches per staged backward");
    p->stage_groups = n_groups;
    return 0;
}
extern "C" int dmvae_plan_grad_buckets(const dmvae_plan* p, int64_t bounds[5]) {
    DMVAE_REQUIRE(p && bounds, "dmvae_plan_grad_buckets: null pointer");
    bounds[0] = 0;                                   // stage 2 completes [bounds[0], bounds[1])  (trunk weights)
    bounds[1] = p->vade ? p->mv.w_off : p->zc.w_off; // stage 1 completes [bounds[1], bounds[2])  (heads weights)
    bounds[2] = p->dec.empty() ? p->out.w_off : p->dec[0].w_off;   // stage 0 completes [bounds[2], bounds[3])  (decoder weights)
    bounds[3] = p->tail_off;                         // [bounds[3], bounds[4]): the tail -- every bias, the prior tables: complete
    bounds[4] = p->param_elems;                      // when the LAST segment has run (each segment writes its layers' biases)
    return 0;
}

extern "C" int dmvae_plan_view(const dmvae_plan* p, const char* name, void** ptr, int64_t* ld, int32_t* dtype) {
    DMVAE_REQUIRE(p && p->bound && name && ptr && ld && dtype, "dmvae_plan_view: null argument / plan not bound");
    const std::string n(name);
    const auto& a = p->a;
    const PAct* v = nullptr;
    PAct half;
    if (p->lab.on && (n == "label_ctl" || n == "label_acc" || n == "label_err")) {      // the label attachment's words: not [Bp][cols] activations
        *ptr = WS(p, n == "label_ctl" ? p->lab.o_ctl : n == "label_acc" ? p->lab.o_acc : p->lab.o_err);
        *ld = n == "label_acc" ? p->lab.acc_elems : 1;
        *dtype = n == "label_ctl" ? DMVAE_F32 : n == "label_acc" ? DMVAE_F64 : DMVAE_I32;
        return 0;
    }
    if (n == "mean") v = &a.mv;
    else if (n == "log_var") { half = a.mv.sub(p->Dp, p->Dp); v = &half; }
    else if (n == "logits") v = &a.lg;
    else if (n == "weights") v = &a.w;
    else if (n == "eval_w" && p->vade) v = &a.lg;      // dmvae_plan_eval_clusters: the averaged responsibilities
    else if (n == "recon") v = &a.recon;
    else if (n == "x") v = &a.xf;
    else if (n == "Z") v = p->cfg.dtype == DMVAE_BF16 ? &a.Zf : &a.Z;
    else if (n == "dxlogits") v = &a.dl;
    else if (n == "moe_P" && p->moe.on) v = &p->moe.P;      // expert outputs (after a training pass: dP, f32)
    else if (n == "moe_pred" && p->moe.on) v = &p->moe.pred;
    else if (n == "moe_acc" && p->moe.on) v = &p->moe.acc;
    else if (n == "moe_dP" && p->moe.on) v = &p->moe.dP;    // the expert layer's weight-gradient operand (act dtype)
    else if (n == "dlogits") v = &a.dlg;                    // act dtype
    else if (n == "gmu") v = &a.gmu;
    else if (n == "hzc" && !p->vade) v = &a.hzc;   // [z-hidden | c-hidden], halves Hp apart
    else if (n.rfind("enc", 0) == 0 && n.size() == 4 && n[3] - '0' < (int)p->enc.size()) v = &a.enc[n[3] - '0'];
    else if (n.rfind("dec", 0) == 0 && n.size() == 4 && n[3] - '0' < (int)p->dec.size()) v = &a.dec[n[3] - '0'];
    else if (n.rfind("conv", 0) == 0 && n.size() == 5 && n[4] - '0' >= 0 && n[4] - '0' < (int)p->conv.size()) {
        const PConv& L = p->conv[n[4] - '0'];       // zero-bordered [B][hw+2][hw+2][cout_ld] relu outputs, at padded pixel 0
        *ptr = rows0(p, L.o_act, L.P, L.cout_ld); *ld = L.cout_ld; *dtype = p->cfg.dtype;
        return 0;
    } else if (n == "flat" && !p->conv.empty()) v = &a.cflat;
    else { set_error("dmvae_plan_view: unknown view '%s'", name); return DMVAE_EINVAL; }
    *ptr = WS(p, *v); *ld = v->ld; *dtype = v->es == 4 ? DMVAE_F32 : DMVAE_BF16;
    return 0;
}
