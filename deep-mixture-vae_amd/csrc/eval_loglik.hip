// Held-out log-likelihood on the device: the importance-weighted bound of Burda et al. (2016) with S draws per row,
//     z_s = mean + exp(log_var / 2) eps_s,   w_s = log p(x | z_s) + log p(z_s) - log q(z_s | x),   L(x) = logsumexp_s w_s - log S
// on the marginal mixture prior p(z) = 1/K sum_k N(z; mu_k, exp(lambda_k)) -- DeepMixtureVAE and VaDE alike (both hold a uniform prior over
// the clusters).  The D log 2 pi terms of log p(z) and log q cancel and are dropped from both.  Three row kernels around the plan's GEMMs
// (dmvae_plan_eval_loglik, api.hip: encoder once, then per draw this file's draw kernel, the decoder, the rows kernel):
//
//   loglik_draw_kernel    geometry of latent_vade_kernel: 16 lanes per row, 16 rows per 256-thread workgroup.  z_s to the plan's Z buffers (act
//                         dtype, and f32 on bf16 plans: the decoder reads the rounded z, the prior and posterior terms the f32 z, as in the
//                         step), pad columns and rows >= n_valid zeroed;  a_s[r] = log p(z_s) - log q_s to the scratch:
//                             log q_s    = -1/2 sum_d (eps_sd^2 + log_var_d)
//                             log p(z_s) = logsumexp_k [ -1/2 sum_d ((z_sd - mu_kd)^2 exp(-lambda_kd) + lambda_kd) ] - log K
//                         The prior tables pass through LDS in tiles of 16 clusters x 64 columns: k tiles outside, d chunks inside, the row's z
//                         whole in LDS (up to D = 764; wider rows are read back from the f32 z the workgroup has just stored) -- no limit on
//                         K or D.  Lane l of a row owns cluster k0 + l of a tile, adds its d in ascending order and keeps a running
//                         (max, scaled sum) over its tiles; the 16 lanes are combined by the xor tree: a fixed order.
//                         eps_s: the caller's [draws][n_valid][ld_eps], or Philox keyed by (seed, counter, stream LOGLIK_PHILOX_STREAM, element
//                         ((s * n_rows + first + r) * D + d)): a function of the row's POSITION in the evaluated order (as eval_clusters.hip).
//   loglik_rows_kernel    one wave per row, 16-byte loads of the f32 logits and targets, columns i < input_dim ONLY (a pad column holds
//                         logit 0 and target 0: -log 2 each).  binary: sum_i (x l - max(l, 0) - log(1 + exp(-|l|))) (minus the step's
//                         sigmoid cross-entropy);  real: -1/2 sum_i (x - l)^2 - I/2 log 2 pi.  Adds a_s[r]; draw 0 initialises the row's
//                         running (max, scaled sum) of the logsumexp over draws, every later draw updates it.
//   loglik_finish_kernel  one workgroup: L_r = m + log(sum) - log S, optionally stored; sum_r L_r and n_valid added into a device double[2]
//                         by a fixed-order tree.  No float atomics: two runs agree bit for bit.
#include "latent_body.h"
#include "eval_loglik.h"

namespace dmvae {

constexpr int LL_RB = 16;          // rows per workgroup
constexpr int LL_KT = 16;          // clusters per table tile: one per lane of a row
constexpr int LL_DC = 64;          // columns per table chunk
constexpr int LL_DCP = LL_DC + 1;
constexpr size_t LL_TABLE_BYTES = sizeof(float) * 3 * LL_KT * LL_DCP;
constexpr size_t LL_LDS_BUDGET = 60 * 1024;

// ZLDS: the rows' z live in LDS ([16][D + 1] behind the table tile); else they are read back from the f32 Z rows this workgroup stored
template <bool ZLDS>
__global__ __launch_bounds__(256) void loglik_draw_kernel(LoglikDrawArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = a.K, D = a.D, DP = D + 1;
    float* tpm = lds;                          // [KT][DCP] prior means
    float* tip = tpm + LL_KT * LL_DCP;         // [KT][DCP] exp(-prior_log_var)
    float* tlv = tip + LL_KT * LL_DCP;         // [KT][DCP] prior_log_var
    float* rz = tlv + LL_KT * LL_DCP;          // [RB][DP] z (ZLDS)

    const int tid = threadIdx.x, lr = tid & 15, rsub = tid >> 4;
    const int b = blockIdx.x * LL_RB + rsub;                    // < B_pad: the grid is B_pad / 16
    const bool valid = b < a.n_valid;
    const uint64_t pos = (uint64_t)a.draw * (uint64_t)a.n_rows + (uint64_t)(a.first + b);

    // reparameterisation: lane owns d = lr + 16 i
    float qs = 0.f;                            // sum_d eps^2 + log_var
    for (int d = lr; d < a.ld_Z; d += 16) {
        float z = 0.f;
        if (valid && d < D) {
            const float mu = a.mean[(int64_t)b * a.ld_mean + d];
            const float lv = a.log_var[(int64_t)b * a.ld_log_var + d];
            const float ep = a.eps ? a.eps[((int64_t)a.draw * a.n_valid + b) * a.ld_eps + d]
                                   : philox_normal_at(a.seed, a.counter, LOGLIK_PHILOX_STREAM, pos * (uint64_t)D + d);
            z = mu + __expf(0.5f * lv) * ep;
            qs += ep * ep + lv;
        }
        if (ZLDS && d < D) rz[rsub * DP + d] = z;
        if (a.act_dtype == DMVAE_BF16) reinterpret_cast<bf16_t*>(a.Z_act)[(int64_t)b * a.ld_Z + d] = f2bf(z);     // pad columns, pad rows: zeros
        else reinterpret_cast<float*>(a.Z_act)[(int64_t)b * a.ld_Z + d] = z;
        if (a.Z_f32 && d < a.ld_Zf) a.Z_f32[(int64_t)b * a.ld_Zf + d] = z;
    }
    qs = row_sum16(qs);
    const float* zrow = ZLDS ? rz + rsub * DP
                             : (a.Z_f32 ? a.Z_f32 + (int64_t)b * a.ld_Zf : reinterpret_cast<const float*>(a.Z_act) + (int64_t)b * a.ld_Z);

    // log p(z): k tiles outside, d chunks inside; this lane's running (max, scaled sum) over its clusters
    float m_l = -INFINITY, s_l = 0.f;
    for (int k0 = 0; k0 < K; k0 += LL_KT) {
        const int kk = min(LL_KT, K - k0);
        float su = 0.f;
        for (int d0 = 0; d0 < D; d0 += LL_DC) {
            const int dc = min(LL_DC, D - d0);
            __syncthreads();                   // the tile's last readers are done (first trip: the rows' z are written, in LDS or in global memory)
            for (int idx = tid; idx < kk * dc; idx += 256) {
                const int k = idx / dc, d = idx - k * dc;
                const int64_t g = (int64_t)(k0 + k) * D + d0 + d;
                const float lam = a.prior_log_vars[g];
                tpm[k * LL_DCP + d] = a.prior_means[g];
                tip[k * LL_DCP + d] = __expf(-lam);
                tlv[k * LL_DCP + d] = lam;
            }
            __syncthreads();
            if (lr < kk) {
                const float* pm = tpm + lr * LL_DCP;
                const float* ip = tip + lr * LL_DCP;
                const float* pl = tlv + lr * LL_DCP;
                const float* zz = zrow + d0;
#pragma unroll 4
                for (int d = 0; d < dc; ++d) {
                    const float dz = zz[d] - pm[d];
                    su += dz * dz * ip[d] + pl[d];
                }
            }
        }
        if (lr < kk) {
            const float u = -0.5f * su;
            if (u > m_l) { s_l = s_l * __expf(m_l - u) + 1.f; m_l = u; }
            else s_l += __expf(u - m_l);
        }
    }
    const float m = row_max16(m_l);                                   // K >= 1: lane 0 holds a cluster, m is finite
    const float s = row_sum16(s_l * __expf(m_l - m));                 // (a lane without a cluster: 0 * exp(-inf) = 0)
    if (valid && lr == 0) a.a_out[b] = (m + __logf(s) - __logf((float)K)) + 0.5f * qs;
}

// recon_kind 0 binary, 1 real (dmvae_config.input_type)
__global__ __launch_bounds__(256) void loglik_rows_kernel(const float* logits, const float* x, int64_t ld, int I, int n_valid, int recon_kind, int draw,
                                                          const float* a_s, float* run_m, float* run_s) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_valid) return;                  // (the whole wave)
    const float* lrow = logits + (int64_t)r * ld;
    const float* xrow = x + (int64_t)r * ld;
    float acc = 0.f;
    for (int c = lane * 4; c < I; c += 256) {  // ld is a multiple of 64 >= I: the quad lies inside the row
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(lrow + c);
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(xrow + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float l = l4[j], t = x4[j];
            float v;
            if (recon_kind == 0) v = t * l - fmaxf(l, 0.f) - __logf(1.f + __expf(-fabsf(l)));
            else { const float df = t - l; v = -0.5f * df * df; }
            acc += (c + j < I) ? v : 0.f;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        if (recon_kind != 0) acc -= 0.5f * (float)I * 1.8378770664093453f;      // log 2 pi
        const float w = acc + a_s[r];
        if (draw == 0) { run_m[r] = w; run_s[r] = 1.f; }
        else {
            const float m = run_m[r], s = run_s[r];
            if (w > m) { run_s[r] = s * expf(m - w) + 1.f; run_m[r] = w; }
            else run_s[r] = s + expf(w - m);
        }
    }
}

__global__ __launch_bounds__(256) void loglik_finish_kernel(const float* run_m, const float* run_s, int n_valid, int draws, float* row_ll, double* acc) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const float logS = logf((float)draws);
    double t = 0.0;
    for (int r = tid; r < n_valid; r += 256) {
        const float L = run_m[r] + logf(run_s[r]) - logS;
        if (row_ll) row_ll[r] = L;
        t += (double)L;
    }
    red[tid] = t;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) { acc[0] += red[0]; acc[1] += (double)n_valid; }
}

#define LL_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int64_t loglik_ws_bytes(int B_pad) { return B_pad > 0 ? ((int64_t)3 * B_pad * 4 + 255) / 256 * 256 : 0; }

int loglik_draw_launch(hipStream_t s, const LoglikDrawArgs& a) {
    LL_REQUIRE(a.D >= 1 && a.K >= 1 && a.mean && a.log_var && a.prior_means && a.prior_log_vars && a.Z_act && a.a_out, "loglik_draw: null pointer / D=%d K=%d", a.D, a.K);
    LL_REQUIRE(a.B_pad > 0 && a.B_pad % LL_RB == 0 && a.n_valid >= 0 && a.n_valid <= a.B_pad, "loglik_draw: B_pad=%d (a multiple of 16) must hold n_valid=%d rows", a.B_pad, a.n_valid);
    LL_REQUIRE(a.draw >= 0 && a.first >= 0 && a.first + a.n_valid <= a.n_rows, "loglik_draw: draw=%d, rows [%lld, %lld + %d) of %lld", a.draw, (long long)a.first,
               (long long)a.first, a.n_valid, (long long)a.n_rows);
    LL_REQUIRE(a.ld_mean >= a.D && a.ld_log_var >= a.D && a.ld_Z >= a.D && (!a.Z_f32 || a.ld_Zf >= a.D) && (!a.eps || a.ld_eps >= a.D), "loglik_draw: leading dimension too small");
    LL_REQUIRE(a.Z_f32 || a.act_dtype != DMVAE_BF16, "loglik_draw: a bf16 Z needs its f32 copy");
    const size_t zb = sizeof(float) * LL_RB * ((size_t)a.D + 1);
    const bool zlds = LL_TABLE_BYTES + zb <= LL_LDS_BUDGET;
    const int nblk = a.B_pad / LL_RB;
    const double n = a.n_valid;
    ProfScope ps(s, "loglik_draw", 4.0 * n * (double)a.K * a.D, 4.0 * (n * (3.0 * a.D + 1.0 + (a.eps ? a.D : 0.0)) + 2.0 * a.K * a.D * nblk));
    if (zlds) DMVAE_LAUNCH(loglik_draw_kernel<true>, dim3(nblk), dim3(256), LL_TABLE_BYTES + zb, s, a);
    else DMVAE_LAUNCH(loglik_draw_kernel<false>, dim3(nblk), dim3(256), LL_TABLE_BYTES, s, a);
    return check_launch("loglik_draw");
}

int loglik_rows_launch(hipStream_t s, const float* logits, const float* x, int64_t ld, int I, int n_valid, int recon_kind, int draw,
                       const float* a_s, float* run_m, float* run_s) {
    LL_REQUIRE(logits && x && a_s && run_m && run_s && I >= 1 && ld >= I && ld % 4 == 0 && n_valid >= 0 && draw >= 0, "loglik_rows: null pointer / I=%d ld=%lld", I, (long long)ld);
    LL_REQUIRE(((uintptr_t)logits | (uintptr_t)x) % 16 == 0, "loglik_rows: logits / targets must be 16-byte aligned");
    if (n_valid == 0) return 0;
    ProfScope ps(s, "loglik_rows", 8.0 * n_valid * (double)I, 4.0 * n_valid * (2.0 * I + 3.0));
    DMVAE_LAUNCH(loglik_rows_kernel, dim3((n_valid + 3) / 4), dim3(256), 0, s, logits, x, ld, I, n_valid, recon_kind, draw, a_s, run_m, run_s);
    return check_launch("loglik_rows");
}

int loglik_finish_launch(hipStream_t s, const float* run_m, const float* run_s, int n_valid, int draws, float* row_ll, double* acc) {
    LL_REQUIRE(run_m && run_s && acc && n_valid >= 0 && draws >= 1, "loglik_finish: null pointer / draws=%d", draws);
    if (n_valid == 0) return 0;
    ProfScope ps(s, "loglik_finish", 4.0 * n_valid, 4.0 * n_valid * 3.0);
    DMVAE_LAUNCH(loglik_finish_kernel, dim3(1), dim3(256), 0, s, run_m, run_s, n_valid, draws, row_ll, acc);
    return check_launch("loglik_finish");
}

}  // namespace dmvae
