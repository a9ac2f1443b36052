// Large-table form of VaDE's latent stage (mode 2; the one-kernel form and the formulas of the stage: latent_vade.hip, which
// keeps both prior tables whole in LDS and so stops at 60 KiB).  The (row, cluster, dimension) contractions as exact-f32 MFMA
// GEMMs (v_mfma_f32_16x16x4_f32 through gemm_f32.hip, as latent_mfma.hip does for DMVAE), taken twice -- once for the mean,
// once for the sample.  With ip = exp(-plv), pm = prior mean, e = exp(lv), mu = mean, z = mu + exp(lv / 2) eps,
// cl = eps / 2 exp(lv / 2), r = kl_ratio, c2_k = sum_d pm^2 ip, ck_k = sum_d plv, over 2 B STACKED rows (mean rows, then
// sample rows):
//
//   X   = [e + mu^2 | mu | 1] ; [z^2 | z | 1]                                        [2B][2D + 64]   (vade_pre)
//   S   = X . [ip | -2 pm ip]^T          S_mu + c2 + ck - sum_d lv - D = T,   u = -1/2 (S_z + c2 + ck)            (G2)
//   gamma = softmax_k(u),  G = r/B (T/2 + log(gamma + e0) + gamma / (gamma + e0) + log K),  du = gamma (G - sum gamma G)
//   (G taken relative to the row's smallest T / 2, without log K: the same du, see vade_rows),
//   KL_Z, KL_C                                                                       W2 = gamma ; du  [2B][K] (vade_rows)
//   [A | C] ; [A_u | C_u] = W2 . [ip | pm ip]                                                                     (G1)
//         -> dZ_lat = -(z A_u - C_u),  gmu = r/B (mu A - C) + dZ_lat,  glv = r/2B (e A - 1) + dZ_lat cl    (vade_post)
//   G_gamma = gamma^T . [e + mu^2 | mu | 1],  G_u = du^T . [z^2 | z | 1]     ONE problem contracted over the 2B stacked rows
//         whose K slices never straddle row B: the first half of its slabs sums to G_gamma, the second to G_u    (G3)
//         -> d pm  = -r/B ip (Gg_mu - pm Wsum) + ip (Gu_z - pm Usum)
//            d plv = r/2B (Wsum - ip (Gg_e - 2 pm Gg_mu + pm^2 Wsum)) + 1/2 (ip (Gu_zz - 2 pm Gu_z + pm^2 Usum) - Usum)
//
// mu, z and pm above are all taken from one origin m0 (vade_origin_kernel: only differences enter the stage; the expansion is what the
// shift is for); Z as the caller sees it is not shifted.
// (oracle/dmvae_oracle.py::vade_latent_backward with the squares expanded; tests/test_vade_large_host.py holds the algebra.)
// Launches: vade_pre (+ the tables as extra workgroups), G2, vade_rows, G1 + G3 as one grid, vade_post (+ the prior-table
// gradients as extra workgroups).  The expanded squares cancel: bf16 operands are not an option (latent_mfma.hip).  The
// [B, K, D] tensor is never formed, nothing is sized blocks x K x D: the scratch is linear in B D + B K + K D.  No float
// atomics; slabs are summed in ascending order; the scores' slabs, c2 and ck are added in double (u ~ -D: a float sum would
// cost the softmax half an ulp of D per addition).  The loss partials are written for latent_vade_nblocks() blocks as in the
// one-kernel form, the prior-table gradient arrives COMPLETE in row 0 of dprior_partials (one partial set).
// Device noise: latent_mfma.hip's keying -- one Philox block per four columns of a row, block index b * (Dp / 4) + d / 4,
// normal d & 3 -- NOT latent_vade.hip's philox_normal_at(b * D + d): a different, equally valid stream.
//
// The evaluation (eval_clusters.hip: averaged responsibilities of `draws` samples) at these shapes is the forward half per
// draw: vade_eval_z, G2 on the sample rows alone, vade_eval_rows; its noise is keyed exactly as vade_eval_kernel keys it.
// The quad code of vade_pre and vade_eval_z, the slab sums and the prior-table gradients are latent_mfma_rows.h's, shared with DMVAE's form;
// the scratch head and its slice rule are latent_tables.h's.  What stays different from latent_mfma.hip on purpose: one quad per lane and trip,
// the scores added in double with an extra pass over the slabs, the origin.
#include "eval_clusters.h"
#include "latent_mfma_rows.h"

namespace dmvae {

struct VadeMfmaWs : LatentWsHead {        // float offsets into the caller's scratch; nsplit counts the slices of EACH half of G3
    int64_t X, S, RL, W2, AC, G, m0, total;
};
static VadeMfmaWs vade_mfma_layout(int Bp, int D, int K) {
    VadeMfmaWs w;
    WsTake take = latent_ws_head(w, Bp, D, K, 2, 16);
    w.X = take((int64_t)2 * Bp * w.XW); w.S = take((int64_t)w.nsplit_s * 2 * Bp * w.Kp); w.RL = take(Bp);
    w.W2 = take((int64_t)2 * Bp * w.Kp); w.AC = take((int64_t)2 * Bp * 2 * w.Dp);
    w.G = take((int64_t)2 * w.nsplit * w.Kp * w.XW);
    w.m0 = take(w.Dp);
    w.total = take.o;
    return w;
}

static int g_vade_force_mfma = 0;               // debug knob (dmvae_debug_set_knob 22): this form at every shape (without the caller's scratch: DMVAE_EINVAL)
void latent_vade_force_mfma(int v) { g_vade_force_mfma = v; }
bool latent_vade_mfma_needed(int D, int K) { return latent_vade_lds_bytes(D, K) > 60 * 1024; }
bool latent_vade_mfma_forced() { return g_vade_force_mfma != 0; }
int64_t latent_vade_mfma_ws_bytes(int B_pad, int D, int K, int* n_slabs) {
    const VadeMfmaWs w = vade_mfma_layout(B_pad, D, K);
    if (n_slabs) *n_slabs = 2 * w.nsplit;
    return 4 * w.total;
}

struct VadeMfmaArgs {
    dmvae_latent_args a;
    VadeMfmaWs w;
    float* ws;
};

// The origin of every expanded product: m0_d = sum_k w_kd pm_kd / sum_k w_kd with w = ip^2 (taken relative to the dimension's largest, so
// that it cannot overflow) -- the point that makes the GEMM operand column (pm - m0) ip smallest in the least-squares sense.  The stage is
// invariant under a common shift of mean, z and the prior means (only differences enter it), but the expanded squares are not: with pm ~ 1
// and ip = 1e6 (a cluster collapsed onto the reg_covar floor, a dead latent dimension) z^2 ip - 2 z pm ip + pm^2 ip cancels 2.5e8 down
// to D at D = 256 and the scores of the rows ON that cluster were off by tens of nats; from m0 that cluster's pm is ~ 0 and its rows' z is
// a small DIFFERENCE taken first.  One thread per dimension, clusters in ascending order: every launch computes the same bits.
__global__ __launch_bounds__(256) void vade_origin_kernel(const float* __restrict__ pm, const float* __restrict__ plv, int K, int D, int Dp, float* __restrict__ m0) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= Dp) return;
    float v = 0.f;
    if (d < D) {
        float mn = INFINITY;
        for (int k = 0; k < K; ++k) mn = fminf(mn, plv[(int64_t)k * D + d]);
        float s1 = 0.f, s2 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float wk = __expf(2.f * (mn - plv[(int64_t)k * D + d]));
            s1 += wk * pm[(int64_t)k * D + d];
            s2 += wk;
        }
        v = s1 / s2;
    }
    m0[d] = v;
}
static int vade_origin_launch(hipStream_t s, const float* pm, const float* plv, int K, int D, const VadeMfmaWs& w, float* ws) {
    return latent_launch_rows(s, "vade_origin", 16.0 * K * D, vade_origin_kernel, (w.Dp + 255) / 256, pm, plv, K, D, w.Dp, ws + w.m0);
}

__global__ __launch_bounds__(256) void vade_tables_kernel(const float* pm, const float* plv, int K, int D, VadeMfmaWs w, float* ws) {
    __shared__ float tred[8];
    latent_tables_block((int)blockIdx.x, pm, plv, ws + w.m0, K, D, w, ws, tred);
}

// ---- rows, before the GEMMs.  16 lanes per row, 16 rows per 256-thread block; a lane owns quads of columns.
__global__ __launch_bounds__(256) void vade_pre_kernel(VadeMfmaArgs L, int nrow_blocks) {
    const dmvae_latent_args& a = L.a;
    if ((int)blockIdx.x >= nrow_blocks) {        // extra workgroups: the prior tables as GEMM operands
        __shared__ float tred[8];
        latent_tables_block((int)blockIdx.x - nrow_blocks, a.prior_means, a.prior_log_vars, L.ws + L.w.m0, a.K, a.D, L.w, L.ws, tred);
        return;
    }
    const int lane16 = threadIdx.x & 15, rsub = threadIdx.x >> 4;
    const int D = a.D, Dp = L.w.Dp, XW = L.w.XW;
    const dmvae_state* st = reinterpret_cast<const dmvae_state*>(a.state);
    const uint64_t nstep = st ? st->noise_step : a.noise_step;
    const int b = blockIdx.x * 16 + rsub;
    const bool valid = b < a.B;
    const int64_t br = valid ? b : 0;            // loads of a pad row read row 0 (unconditional loads; the values are not used)
    float* Xm = L.ws + L.w.X + (int64_t)b * XW;
    float* Xz = L.ws + L.w.X + ((int64_t)a.B_pad + b) * XW;
    const float* mrow = a.mean + br * a.ld_mean;
    const float* vrow = a.log_var + br * a.ld_log_var;
    const float* erow = a.eps ? a.eps + br * a.ld_eps : nullptr;
    const bool vec = latent_quads_aligned(a);
    float lvsum = 0.f;
    for (int q4 = lane16; q4 < Dp / 4; q4 += 16) {
        const int d0 = 4 * q4;
        float mu[4], lv[4], ep[4];
        load_quad(mrow, vrow, erow, vec, d0, D, mu, lv, ep);
        const bool ok[4] = {valid && d0 < D, valid && d0 + 1 < D, valid && d0 + 2 < D, valid && d0 + 3 < D};
        if (ok[0] && !a.eps) philox_normal4(a.seed, nstep, 0u, (uint64_t)b * (Dp / 4) + q4, ep);
        const float4 o4 = *reinterpret_cast<const float4*>(L.ws + L.w.m0 + d0);      // the origin of the GEMM operands (vade_origin_kernel); Z itself is not shifted
        const float org[4] = {o4.x, o4.y, o4.z, o4.w};
        float z[4], cl[4], x1[4], zs[4];
        reparam_quad(mu, lv, ep, ok, org, z, cl, x1, zs, lvsum);
        *reinterpret_cast<float4*>(Xm + d0) = make_float4(x1[0], x1[1], x1[2], x1[3]);
        *reinterpret_cast<float4*>(Xm + Dp + d0) = make_float4(mu[0], mu[1], mu[2], mu[3]);
        *reinterpret_cast<float4*>(Xz + d0) = make_float4(zs[0] * zs[0], zs[1] * zs[1], zs[2] * zs[2], zs[3] * zs[3]);
        *reinterpret_cast<float4*>(Xz + Dp + d0) = make_float4(zs[0], zs[1], zs[2], zs[3]);
        store_z_quad(a, b, d0, vec, z, cl);
    }
    zero_z_tail(a, b, Dp, lane16);
    write_ones_column(Xm + 2 * Dp, lane16, valid);      // G3 then also yields sum_b gamma and sum_b du
    write_ones_column(Xz + 2 * Dp, lane16, valid);
    lvsum = row_sum16(lvsum);
    if (lane16 == 0) L.ws[L.w.RL + b] = lvsum;
}

// S_k + c2_k + ck_k of four clusters k0 .. k0 + 3 of one row from the K-slice slabs, in double (slabs in ascending order).  k0 < Kp: the pad
// columns of S, c2 and ck exist (zeros)
__device__ __forceinline__ void vade_score4(const float* S0, int64_t sstr, int nss, const float* c2, const float* ck, int k0, double v[4]) {
    slab_sum<double, 4, true>(S0, sstr, nss, &k0, v);
    const float4 p = *reinterpret_cast<const float4*>(c2 + k0), q = *reinterpret_cast<const float4*>(ck + k0);
    v[0] = v[0] + (double)p.x + (double)q.x; v[1] = v[1] + (double)p.y + (double)q.y;
    v[2] = v[2] + (double)p.z + (double)q.z; v[3] = v[3] + (double)p.w + (double)q.w;
}

// one row of responsibilities to the caller's [rows][ld] array: 16 bytes where the quad is whole and aligned
__device__ __forceinline__ void vade_store_w4(float* row, bool vecw, int k0, int K, const float g[4]) {
    if (vecw && k0 + 4 <= K) *reinterpret_cast<float4*>(row + k0) = make_float4(g[0], g[1], g[2], g[3]);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k0 + j < K) row[k0 + j] = g[j];
    }
}

// ---- rows, between G2 and G1 / G3: responsibilities, both KL terms, dL/du.  A lane owns the QUADS of clusters k0 = 4 (lane16 + 16 i): every access
// to the scratch is 16 bytes wide.  A row's W2 entries are its staging for T, then G (each lane reads back only what it wrote).
__global__ __launch_bounds__(256) void vade_rows_kernel(VadeMfmaArgs L) {
    const dmvae_latent_args& a = L.a;
    const int lane16 = threadIdx.x & 15, rsub = threadIdx.x >> 4;
    const int K = a.K, Kp = L.w.Kp, nss = L.w.nsplit_s;
    const dmvae_state* st = reinterpret_cast<const dmvae_state*>(a.state);
    const float klr = st ? st->kl_ratio : a.kl_ratio;
    const float rB = klr * a.inv_B, logK = __logf((float)K);
    const int b = blockIdx.x * 16 + rsub;
    const bool valid = b < a.B;
    const int64_t sstr = (int64_t)2 * a.B_pad * Kp;
    const float* Sm = L.ws + L.w.S + (int64_t)b * Kp;
    const float* Sz = L.ws + L.w.S + ((int64_t)a.B_pad + b) * Kp;
    const float* c2 = L.ws + L.w.c2;
    const float* ck = L.ws + L.w.ck;
    float* gam = L.ws + L.w.W2 + (int64_t)b * Kp;
    float* dus = L.ws + L.w.W2 + ((int64_t)a.B_pad + b) * Kp;
    const float base = L.ws[L.w.RL + b] + (float)a.D;
    const bool vecw = a.weights && a.ld_w % 4 == 0 && (reinterpret_cast<uintptr_t>(a.weights) & 15) == 0;
    __shared__ float red[32];

    double mxd = -INFINITY;
    float tmin = INFINITY;
    for (int k0 = 4 * lane16; k0 < K; k0 += 64) {
        double uz[4], sm[4];
        vade_score4(Sz, sstr, nss, c2, ck, k0, uz);
        vade_score4(Sm, sstr, nss, c2, ck, k0, sm);
        float T[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = k0 + j < K;
            T[j] = in ? (float)sm[j] - base : 0.f;
            if (in) { mxd = fmax(mxd, -0.5 * uz[j]); tmin = fminf(tmin, T[j]); }
        }
        *reinterpret_cast<float4*>(dus + k0) = make_float4(T[0], T[1], T[2], T[3]);      // T_k for now
    }
    mxd = row_max16(mxd); tmin = row_min16(tmin);
    float se = 0.f;
    for (int k0 = 4 * lane16; k0 < K; k0 += 64) {
        double uz[4];
        vade_score4(Sz, sstr, nss, c2, ck, k0, uz);
        float ex[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ex[j] = k0 + j < K ? __expf((float)(-0.5 * uz[j] - mxd)) : 0.f;
            se += ex[j];
        }
        *reinterpret_cast<float4*>(gam + k0) = make_float4(ex[0], ex[1], ex[2], ex[3]);
    }
    se = row_sum16(se);
    float sgG = 0.f, klz = 0.f, klc = 0.f;
    for (int k0 = 4 * lane16; k0 < K; k0 += 64) {
        const float4 e4 = *reinterpret_cast<const float4*>(gam + k0), T4 = *reinterpret_cast<const float4*>(dus + k0);
        const float ex[4] = {e4.x, e4.y, e4.z, e4.w}, T[4] = {T4.x, T4.y, T4.z, T4.w};
        float g[4], G[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = k0 + j < K;
            g[j] = valid && in ? ex[j] / se : 0.f;
            const float lg = __logf(g[j] + 1e-20f);
            // G up to a constant of the row: du = gamma (G - sum gamma G) does not see it in exact arithmetic, but sum_k gamma_k is 1 only to
            // an ulp, and sum_k du_k = (1 - sum gamma) sum gamma G then leaks into dZ_lat times z.  T ~ D makes G ~ r/B D/2: taken relative
            // to the row's smallest T (and without log K) the leak is of the size of the DIFFERENCES of G, as du itself.
            G[j] = in ? rB * (0.5f * (T[j] - tmin) + lg + g[j] / (g[j] + 1e-20f)) : 0.f;
            if (in) {
                sgG += g[j] * G[j];
                klz += 0.5f * g[j] * T[j];
                klc += g[j] * (lg + logK);
            }
        }
        *reinterpret_cast<float4*>(gam + k0) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(dus + k0) = make_float4(G[0], G[1], G[2], G[3]);      // G for now
        if (a.weights) vade_store_w4(a.weights + (int64_t)b * a.ld_w, vecw, k0, K, g);
    }
    sgG = row_sum16(sgG); klz = row_sum16(klz); klc = row_sum16(klc);
    for (int k0 = 4 * lane16; k0 < Kp; k0 += 64) {
        float4 du = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 < K) {                                                        // (gamma of a pad cluster inside the quad is already 0)
            const float4 g4 = *reinterpret_cast<const float4*>(gam + k0), G4 = *reinterpret_cast<const float4*>(dus + k0);
            du.x = g4.x * (G4.x - sgG); du.y = g4.y * (G4.y - sgG); du.z = g4.z * (G4.z - sgG); du.w = g4.w * (G4.w - sgG);
        } else *reinterpret_cast<float4*>(gam + k0) = du;                    // pad clusters: zero rows of G3, zero terms of G1
        *reinterpret_cast<float4*>(dus + k0) = du;
    }
    if (lane16 == 0) { red[rsub] = valid ? klz : 0.f; red[16 + rsub] = valid ? klc : 0.f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float z = 0.f, c = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { z += red[i]; c += red[16 + i]; }
        a.loss_partials[2 * blockIdx.x] = z;
        a.loss_partials[2 * blockIdx.x + 1] = c;
    }
}

// ---- rows, after the GEMMs; workgroups >= nrow_blocks: the prior-table gradients from the G slabs
__global__ __launch_bounds__(256) void vade_post_kernel(VadeMfmaArgs L, int nrow_blocks) {
    const dmvae_latent_args& a = L.a;
    const int D = a.D, K = a.K, Dp = L.w.Dp, XW = L.w.XW;
    const dmvae_state* st = reinterpret_cast<const dmvae_state*>(a.state);
    const float klr = st ? st->kl_ratio : a.kl_ratio;
    const float rB = klr * a.inv_B, rB2 = 0.5f * rB;
    if ((int)blockIdx.x >= nrow_blocks) {      // (the tables' origin: G holds sums of the shifted mean and z)
        prior_grad_from_slabs<true>(L.w, L.ws, L.w.G, a.prior_means, L.ws + L.w.m0, K, D, rB, a.dprior_partials, nrow_blocks);
        return;
    }
    const int lane16 = threadIdx.x & 15, rsub = threadIdx.x >> 4;
    const int b = blockIdx.x * 16 + rsub;
    const bool valid = b < a.B;
    const int64_t br = valid ? b : 0;
    const float* ACm = L.ws + L.w.AC + (int64_t)b * 2 * Dp;
    const float* ACu = L.ws + L.w.AC + ((int64_t)a.B_pad + b) * 2 * Dp;
    const float* Xm = L.ws + L.w.X + (int64_t)b * XW;
    const float* Xz = L.ws + L.w.X + ((int64_t)a.B_pad + b) * XW;
    const float* vrow = a.log_var + br * a.ld_log_var;
    const float* crow = a.clv + (int64_t)b * a.ld_g;      // what vade_pre wrote (columns < D of every row)
    const bool vec = D % 4 == 0 && a.ld_log_var % 4 == 0 && a.ld_g % 4 == 0;
    for (int q4 = lane16; q4 < (D + 3) / 4; q4 += 16) {
        const int d0 = 4 * q4;
        const float4 A4 = *reinterpret_cast<const float4*>(ACm + d0), C4 = *reinterpret_cast<const float4*>(ACm + Dp + d0);
        const float4 U4 = *reinterpret_cast<const float4*>(ACu + d0), V4 = *reinterpret_cast<const float4*>(ACu + Dp + d0);
        const float4 M4 = *reinterpret_cast<const float4*>(Xm + Dp + d0), Z4 = *reinterpret_cast<const float4*>(Xz + Dp + d0);
        const float A[4] = {A4.x, A4.y, A4.z, A4.w}, Cc[4] = {C4.x, C4.y, C4.z, C4.w}, Au[4] = {U4.x, U4.y, U4.z, U4.w}, Cu[4] = {V4.x, V4.y, V4.z, V4.w};
        const float mu[4] = {M4.x, M4.y, M4.z, M4.w}, z[4] = {Z4.x, Z4.y, Z4.z, Z4.w};
        float lv[4], cl[4];
        if (vec) {
            const float4 l4 = *reinterpret_cast<const float4*>(vrow + d0), c4 = *reinterpret_cast<const float4*>(crow + d0);
            lv[0] = l4.x; lv[1] = l4.y; lv[2] = l4.z; lv[3] = l4.w;
            cl[0] = c4.x; cl[1] = c4.y; cl[2] = c4.z; cl[3] = c4.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int off = d0 + j < D ? d0 + j : 0;
                lv[j] = vrow[off]; cl[j] = crow[off];
            }
        }
        float gm[4], gl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dzl = -(z[j] * Au[j] - Cu[j]);
            gm[j] = valid ? rB * (mu[j] * A[j] - Cc[j]) + dzl : 0.f;
            gl[j] = valid ? rB2 * (__expf(lv[j]) * A[j] - 1.f) + dzl * cl[j] : 0.f;
        }
        if (vec) {
            *reinterpret_cast<float4*>(a.gmu + (int64_t)b * a.ld_g + d0) = make_float4(gm[0], gm[1], gm[2], gm[3]);
            *reinterpret_cast<float4*>(a.glv + (int64_t)b * a.ld_g + d0) = make_float4(gl[0], gl[1], gl[2], gl[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (d0 + j < D) {
                    a.gmu[(int64_t)b * a.ld_g + d0 + j] = gm[j];
                    a.glv[(int64_t)b * a.ld_g + d0 + j] = gl[j];
                }
        }
    }
}

static int vade_score_gemm(hipStream_t s, const VadeMfmaWs& w, float* ws, int rows) {
    // G2 (dX layout): rows x [2 Dp] . ([Kp] x [2 Dp])^T, its K slices into slabs
    const GemmArgs g2 = f32_problem(rows, w.Kp, 2 * w.Dp, ws + w.X, w.XW, ws + w.T2, 2 * w.Dp, ws + w.S, w.Kp, w.nsplit_s, (int64_t)rows * w.Kp);
    return gemm_f32_dispatch(s, DMVAE_GEMM_DX, g2, w.nsplit_s);
}

int latent_vade_mfma_launch(hipStream_t s, const dmvae_latent_args* a, float* ws, int64_t ws_bytes) {
    const VadeMfmaWs w = vade_mfma_layout(a->B_pad, a->D, a->K);
    if (!ws || 4 * w.total > ws_bytes) {
        set_error("dmvae_latent_fwd (VaDE): K=%d D=%d takes the large-table form, which needs mfma_ws of dmvae_latent_vade_ws_bytes() = %lld bytes (got %lld)",
                  a->K, a->D, (long long)(4 * w.total), (long long)(ws ? ws_bytes : 0));
        return DMVAE_EINVAL;
    }
    VadeMfmaArgs L;
    L.a = *a; L.w = w; L.ws = ws;
    const int nrb = a->B_pad / 16, Bp2 = 2 * a->B_pad;
    const double BD = (double)a->B * a->D, BK = (double)a->B * a->K;
    int rc = vade_origin_launch(s, a->prior_means, a->prior_log_vars, a->K, a->D, w, ws);
    if (rc) return rc;
    // the prior-table operands ride as Kp extra workgroups of the row kernel
    rc = latent_launch_rows(s, "vade_pre", 4.0 * (BD * (2.0 + (a->eps ? 1.0 : 0.0) + 4.0 + 2.0 + 1.0)) + 16.0 * a->K * a->D, vade_pre_kernel, nrb + w.Kp, L, nrb);
    if (rc) return rc;
    {
        ProfScope ps(s, "vade_gemm_f32", 2.0 * Bp2 * (double)w.Kp * 2.0 * w.Dp, 4.0 * Bp2 * (2.0 * w.Dp + (double)w.nsplit_s * w.Kp));
        rc = vade_score_gemm(s, w, ws, Bp2);
    }
    if (rc) return rc;
    rc = latent_launch_rows(s, "vade_rows", 4.0 * BK * (4.0 * w.nsplit_s + 3.0), vade_rows_kernel, nrb, L);
    if (rc) return rc;
    {
        ProfScope ps(s, "vade_gemm_f32", 2.0 * Bp2 * (double)w.Kp * (2.0 * w.Dp + w.XW), 4.0 * Bp2 * (2.0 * w.Kp + w.XW + 2.0 * w.Dp));
        // G1 (forward layout) and G3 (dW layout, 2 nsplit batch slices into slabs) read only what the kernels above wrote: one grid
        // (gemm_f32_trio with its dX problem absent)
        const GemmArgs g1 = f32_problem(Bp2, 2 * w.Dp, w.Kp, ws + w.W2, w.Kp, ws + w.T1, 2 * w.Dp, ws + w.AC, 2 * w.Dp, 1, 0);
        const GemmArgs none = f32_problem(0, 64, 16, nullptr, 0, nullptr, 0, nullptr, 0, 1, 0);
        const GemmArgs g3 = f32_problem(w.Kp, w.XW, Bp2, ws + w.W2, w.Kp, ws + w.X, w.XW, ws + w.G, w.XW, 2 * w.nsplit, (int64_t)w.Kp * w.XW);
        rc = gemm_f32_trio(s, g1, 1, none, 1, g3, 2 * w.nsplit);
    }
    if (rc) return rc;
    return latent_launch_rows(s, "vade_post", 4.0 * (BD * (4.0 + 2.0 + 2.0 + 2.0)) + 8.0 * w.nsplit * w.Kp * w.XW, vade_post_kernel,
                              nrb + prior_grad_workgroups(a->K, a->D), L, nrb);
}

// ---- evaluation: averaged responsibilities of `draws` samples (eval_clusters.hip), the forward half per draw
struct VadeEvalMfma {
    VadeEvalArgs a;
    VadeMfmaWs w;
    float* ws;
};

// z of draw j as the rows of G2's A operand: [z^2 | z], pad rows and pad columns zero.  A lane owns quads of columns (16-byte accesses where the
// caller's rows allow it); the noise keeps vade_eval_kernel's per-element keying
__global__ __launch_bounds__(256) void vade_eval_z_kernel(VadeEvalMfma L, int j) {
    const VadeEvalArgs& a = L.a;
    const int lane16 = threadIdx.x & 15, rsub = threadIdx.x >> 4;
    const int D = a.D, Dp = L.w.Dp;
    const int b = blockIdx.x * 16 + rsub;
    const bool valid = b < a.rows.n_valid;
    const int64_t br = valid ? b : 0;
    float* Xz = L.ws + L.w.X + (int64_t)b * L.w.XW;
    const uint64_t pos = (uint64_t)(a.rows.first + b);
    const float* mrow = a.mean + br * a.ld_mean;
    const float* vrow = a.log_var + br * a.ld_log_var;
    const float* erow = a.eps ? a.eps + ((int64_t)j * a.rows.n_valid + br) * a.ld_eps : nullptr;
    const bool vec = D % 4 == 0 && a.ld_mean % 4 == 0 && a.ld_log_var % 4 == 0 && (!a.eps || a.ld_eps % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(a.mean) | reinterpret_cast<uintptr_t>(a.log_var) | reinterpret_cast<uintptr_t>(a.eps)) & 15) == 0;
    for (int d0 = 4 * lane16; d0 < Dp; d0 += 64) {
        float mu[4], lv[4], ep[4];
        load_quad(mrow, vrow, erow, vec, d0, D, mu, lv, ep);
        const bool ok[4] = {valid && d0 < D, valid && d0 + 1 < D, valid && d0 + 2 < D, valid && d0 + 3 < D};
        if (ok[0] && !erow) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                ep[i] = philox_normal_at(a.seed, a.counter, EVAL_PHILOX_STREAM, ((uint64_t)j * (uint64_t)a.rows.n_rows + pos) * (uint64_t)D + (d0 + i < D ? d0 + i : 0));
        }
        const float4 o4 = *reinterpret_cast<const float4*>(L.ws + L.w.m0 + d0);      // from the tables' origin
        const float org[4] = {o4.x, o4.y, o4.z, o4.w};
        float z[4], cl[4], x1[4], zs[4], lvsum = 0.f;
        reparam_quad(mu, lv, ep, ok, org, z, cl, x1, zs, lvsum);      // (only zs is used)
        *reinterpret_cast<float4*>(Xz + d0) = make_float4(zs[0] * zs[0], zs[1] * zs[1], zs[2] * zs[2], zs[3] * zs[3]);
        *reinterpret_cast<float4*>(Xz + Dp + d0) = make_float4(zs[0], zs[1], zs[2], zs[3]);
    }
}

// gamma of draw j added to the row's sum (W2 rows [0, B_pad); rows [B_pad, 2 B_pad) are staging); the last draw writes the average.  Quads of
// clusters per lane, as vade_rows
__global__ __launch_bounds__(256) void vade_eval_rows_kernel(VadeEvalMfma L, int j) {
    const VadeEvalArgs& a = L.a;
    const int lane16 = threadIdx.x & 15, rsub = threadIdx.x >> 4;
    const int K = a.K, Kp = L.w.Kp, nss = L.w.nsplit_s;
    const int b = blockIdx.x * 16 + rsub;
    const bool valid = b < a.rows.n_valid;
    const int64_t sstr = (int64_t)a.B_pad * Kp;
    const float* Sz = L.ws + L.w.S + (int64_t)b * Kp;
    const float* c2 = L.ws + L.w.c2;
    const float* ck = L.ws + L.w.ck;
    float* acc = L.ws + L.w.W2 + (int64_t)b * Kp;
    float* exs = L.ws + L.w.W2 + ((int64_t)a.B_pad + b) * Kp;
    const bool vecw = a.ld_w % 4 == 0 && (reinterpret_cast<uintptr_t>(a.w) & 15) == 0;
    double mxd = -INFINITY;
    for (int k0 = 4 * lane16; k0 < K; k0 += 64) {
        double uz[4];
        vade_score4(Sz, sstr, nss, c2, ck, k0, uz);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (k0 + i < K) mxd = fmax(mxd, -0.5 * uz[i]);
    }
    mxd = row_max16(mxd);
    float se = 0.f;
    for (int k0 = 4 * lane16; k0 < K; k0 += 64) {
        double uz[4];
        vade_score4(Sz, sstr, nss, c2, ck, k0, uz);
        float ex[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ex[i] = k0 + i < K ? __expf((float)(-0.5 * uz[i] - mxd)) : 0.f;
            se += ex[i];
        }
        *reinterpret_cast<float4*>(exs + k0) = make_float4(ex[0], ex[1], ex[2], ex[3]);
    }
    se = row_sum16(se);
    const float nd = (float)a.draws;
    for (int k0 = 4 * lane16; k0 < K; k0 += 64) {
        const float4 e4 = *reinterpret_cast<const float4*>(exs + k0);
        float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j) s4 = *reinterpret_cast<const float4*>(acc + k0);
        const float sum[4] = {s4.x + e4.x / se, s4.y + e4.y / se, s4.z + e4.z / se, s4.w + e4.w / se};
        *reinterpret_cast<float4*>(acc + k0) = make_float4(sum[0], sum[1], sum[2], sum[3]);
        if (j == a.draws - 1 && valid) {
            const float avg[4] = {sum[0] / nd, sum[1] / nd, sum[2] / nd, sum[3] / nd};
            vade_store_w4(a.w + (int64_t)b * a.ld_w, vecw, k0, K, avg);
        }
    }
}

int vade_eval_mfma_launch(hipStream_t s, const VadeEvalArgs& a) {
    const VadeMfmaWs w = vade_mfma_layout(a.B_pad, a.D, a.K);
    VadeEvalMfma L;
    L.a = a; L.w = w; L.ws = a.ws;
    const int nrb = a.B_pad / 16;
    const double n = a.rows.n_valid;
    int rc = vade_origin_launch(s, a.prior_means, a.prior_log_vars, a.K, a.D, w, a.ws);
    if (rc) return rc;
    rc = latent_launch_rows(s, "vade_tables", 24.0 * a.K * a.D, vade_tables_kernel, w.Kp, a.prior_means, a.prior_log_vars, a.K, a.D, w, a.ws);
    if (rc) return rc;
    for (int j = 0; j < a.draws; ++j) {
        if ((rc = latent_launch_rows(s, "vade_eval_z", 4.0 * n * a.D * (4.0 + (a.eps ? 1.0 : 0.0)), vade_eval_z_kernel, nrb, L, j))) return rc;
        {
            ProfScope ps(s, "vade_gemm_f32", 2.0 * a.B_pad * (double)w.Kp * 2.0 * w.Dp, 4.0 * a.B_pad * (2.0 * w.Dp + (double)w.nsplit_s * w.Kp));
            rc = vade_score_gemm(s, w, a.ws, a.B_pad);
        }
        if (rc) return rc;
        if ((rc = latent_launch_rows(s, "vade_eval_rows", 4.0 * n * a.K * (2.0 * w.nsplit_s + 4.0), vade_eval_rows_kernel, nrb, L, j))) return rc;
    }
    return confusion_add_launch(s, a.w, a.ld_w, a.K, a.rows);      // the same arg-max and count as vade_eval_kernel's
}

}  // namespace dmvae
