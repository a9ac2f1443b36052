// Supervised mixture-of-experts head on the DMVAE gate (models.py:10-163 of the reference): the row stage that runs
// behind the latent stage of a step whose plan carries a MoE attachment (dmvae_plan_attach_moe).
//
//   q        = softmax(logits)                         gate, base_models.py:249 (the softmax in BOTH KL modes)
//   P[e,o]   = W[e,o,:] . inp + bias[o,e]              models.py:70-81 (the GEMM in front of this kernel, or -- featLearn, where
//                                                      inp = relu(mean) is a few dozen columns -- this kernel itself)
//   classification (models.py:83-105, 141-144):
//     s_e = softmax_o(P[e,:]),  u = sum_e q_e s_e,  p = u / sum_o u
//     loss_b = -1000 sum_o Y_o log(p_o + 1e-20),  error_b = sum_o |Y_o - onehot(argmax p)_o| / 2
//   regression (models.py:106-113, 145-146):
//     y = sum_e q_e P[e,:],  loss_b = 0.5 sum_o (y_o - Y_o)^2,  error_b = sum_o (y_o - Y_o)^2
// and, with `backward`, every gradient of inv_B * sum_b loss_b:
//     dP (act dtype: the weight-gradient operand; f32 in place of P), dlogits += q (dq - sum q dq) (NOT scaled by kl_ratio),
//     featLearn: inp_act = relu(mean) (the weight-gradient operand) and gmu += (dP . W^T) * [mean > 0].
//
// Layout: 64-thread workgroups, 16 lanes per row (row_sum16 of common.h): lane l owns the outputs o = l, l + 16, l + 32,
// l + 48 (O <= 64) of its row and walks the experts; the per-expert softmax reductions over o are 16-lane shuffles.  Y is read
// through the batch permutation (row r of the batch = Y[perm[first + r]], first = state->batch_cursor * batch when the device
// cursor is used), as the reconstruction epilogue reads its targets.  Per-workgroup loss / error partials go to partials[blk][2]
// and are summed in a fixed order by moe_finalize_kernel: no float atomics.  Rows >= B write zeros.
#include "latent_body.h"
#include "moe_head.h"

namespace dmvae {

constexpr int MOE_ROWS = 4;        // rows per 64-thread workgroup

__device__ __forceinline__ float moe_lbl(const MoeHeadArgs& a, int64_t src, int o) {
    return (src >= 0 && o < a.O) ? a.Y[src * a.O + o] : 0.f;
}

__global__ __launch_bounds__(64) void moe_head_kernel(MoeHeadArgs a) {
    const int lane = threadIdx.x & 15;
    const int grp = threadIdx.x >> 4;
    const int b = blockIdx.x * MOE_ROWS + grp;
    const bool valid = b < a.B;
    const int E = a.E, O = a.O;
    int oo[4];
    bool ov[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { oo[j] = lane + 16 * j; ov[j] = oo[j] < O; }

    // the row's label row through the batch permutation
    int64_t src = -1;
    if (valid) {
        const int64_t first = a.st ? (int64_t)a.st->batch_cursor * a.batch : a.first;
        const int64_t i = first + b;
        src = a.perm ? (int64_t)a.perm[i] : i;
        if (src < 0 || src >= a.n_rows) src = -1;
    }
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = moe_lbl(a, src, oo[j]);

    float* P = a.P + (int64_t)b * a.ldP;

    // featLearn: P = relu(mean) . W + bias computed here; relu(mean) also goes out in act dtype (the weight-gradient operand)
    if (a.featLearn && b < a.B_pad) {
        const float* mrow = a.mean + (int64_t)b * a.ld_mean;
        for (int d = lane; d < a.Dp; d += 16) {
            const float v = (valid && d < a.D) ? fmaxf(mrow[d], 0.f) : 0.f;
            if (a.act_dtype == DMVAE_BF16) reinterpret_cast<bf16_t*>(a.inp_act)[(int64_t)b * a.ld_inp + d] = f2bf(v);
            else reinterpret_cast<float*>(a.inp_act)[(int64_t)b * a.ld_inp + d] = v;
        }
        if (valid) {
            for (int e = 0; e < E; ++e) {
                float acc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = ov[j] ? a.bias[e * O + oo[j]] : 0.f;
                for (int d = 0; d < a.D; ++d) {
                    const float x = fmaxf(mrow[d], 0.f);
                    const float* w = a.W + (int64_t)d * a.ldW + e * O;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ov[j]) acc[j] = fmaf(x, w[oo[j]], acc[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (ov[j]) P[e * O + oo[j]] = acc[j];
            }
        }
    }

    // gate: q = softmax(logits[0:E])
    const float* lg = a.logits + (int64_t)b * a.ld_lg;
    float gmx = -INFINITY, gse = 0.f;
    if (valid) {
        for (int e = lane; e < E; e += 16) gmx = fmaxf(gmx, lg[e]);
        gmx = row_max16(gmx);
        for (int e = lane; e < E; e += 16) gse += __expf(lg[e] - gmx);
        gse = row_sum16(gse);
    }
    const float ginv = valid ? 1.f / gse : 0.f;

    float u[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        for (int e = 0; e < E; ++e) {
            const float q = __expf(lg[e] - gmx) * ginv;
            float pv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) pv[j] = ov[j] ? P[e * O + oo[j]] : -INFINITY;
            if (a.classification) {
                float mx = fmaxf(fmaxf(pv[0], pv[1]), fmaxf(pv[2], pv[3]));
                mx = row_max16(mx);
                float ex[4], se = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) { ex[j] = ov[j] ? __expf(pv[j] - mx) : 0.f; se += ex[j]; }
                se = row_sum16(se);
                const float is = 1.f / se;
#pragma unroll
                for (int j = 0; j < 4; ++j) u[j] += q * (ex[j] * is);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (ov[j]) u[j] += q * pv[j];
            }
        }
    }

    // loss, error, prediction and dLoss/du (g)
    float loss = 0.f, err = 0.f, g[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        if (a.classification) {
            const float U = row_sum16(u[0] + u[1] + u[2] + u[3]);
            const float iU = 1.f / U;
            float pr[4], l = 0.f, bv = -INFINITY;
            int bi = 1 << 30;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pr[j] = u[j] * iU;
                if (ov[j]) {
                    l -= y[j] * __logf(pr[j] + 1e-20f);
                    if (pr[j] > bv) { bv = pr[j]; bi = oo[j]; }      // ascending o within the lane: first index on ties
                }
                if (a.pred && ov[j]) a.pred[(int64_t)b * a.ld_pred + oo[j]] = pr[j];
            }
#pragma unroll
            for (int s = 8; s > 0; s >>= 1) {
                const float ov_ = __shfl_xor(bv, s, 16);
                const int oi = __shfl_xor(bi, s, 16);
                if (ov_ > bv || (ov_ == bv && oi < bi)) { bv = ov_; bi = oi; }
            }
            loss = 1000.f * row_sum16(l);
            float e_ = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (ov[j]) e_ += fabsf(y[j] - (oo[j] == bi ? 1.f : 0.f));
            err = 0.5f * row_sum16(e_);
            // dL/dp_o = -1000 inv_B Y_o / (p_o + 1e-20);  p = u / U:  dL/du_o = (dL/dp_o - sum_j dL/dp_j p_j) / U
            float gp[4], gpp = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { gp[j] = ov[j] ? -1000.f * a.inv_B * y[j] / (pr[j] + 1e-20f) : 0.f; gpp += gp[j] * pr[j]; }
            gpp = row_sum16(gpp);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = ov[j] ? (gp[j] - gpp) * iU : 0.f;
        } else {
            float l = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float r = ov[j] ? u[j] - y[j] : 0.f;
                l += r * r;
                g[j] = a.inv_B * r;
                if (a.pred && ov[j]) a.pred[(int64_t)b * a.ld_pred + oo[j]] = u[j];
            }
            l = row_sum16(l);
            loss = 0.5f * l;
            err = l;
        }
    }

    if (a.backward && b < a.B_pad) {
        // dP and dq per expert; dlogits = q (dq - sum_e q dq)
        float qdq = 0.f;
        for (int e = 0; e < E; ++e) {
            float dp[4] = {0.f, 0.f, 0.f, 0.f};
            float dq = 0.f;
            if (valid) {
                const float q = __expf(lg[e] - gmx) * ginv;
                float pv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) pv[j] = ov[j] ? P[e * O + oo[j]] : -INFINITY;
                if (a.classification) {
                    float mx = fmaxf(fmaxf(pv[0], pv[1]), fmaxf(pv[2], pv[3]));
                    mx = row_max16(mx);
                    float s[4], se = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { s[j] = ov[j] ? __expf(pv[j] - mx) : 0.f; se += s[j]; }
                    se = row_sum16(se);
                    const float is = 1.f / se;
                    float sg = 0.f, dql = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { s[j] *= is; sg += s[j] * g[j]; dql += g[j] * s[j]; }
                    sg = row_sum16(sg);
                    dq = row_sum16(dql);
                    // ds = q g;  dP = s (ds - sum s ds) = q s (g - sum s g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) dp[j] = ov[j] ? q * s[j] * (g[j] - sg) : 0.f;
                } else {
                    float dql = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { if (ov[j]) dql += pv[j] * g[j]; dp[j] = ov[j] ? q * g[j] : 0.f; }
                    dq = row_sum16(dql);
                }
                qdq += q * dq;
            }
            // dP: f32 in place of P (featLearn reads it below), act dtype for the weight gradient (zeros in rows >= B)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!ov[j]) continue;
                const int c = e * O + oo[j];
                if (valid) P[c] = dp[j];
                if (a.act_dtype == DMVAE_BF16) reinterpret_cast<bf16_t*>(a.dP_act)[(int64_t)b * a.ld_dP + c] = f2bf(dp[j]);
                else reinterpret_cast<float*>(a.dP_act)[(int64_t)b * a.ld_dP + c] = dp[j];
            }
            if (lane == (e & 15) && valid) a.dq_ws[(int64_t)b * a.ld_dq + e] = dq;
        }
        // dlogits += q (dq - sum q dq): the lane that stored dq_e adds it (its own earlier store: no barrier needed)
        if (valid) {
            for (int e = lane; e < E; e += 16) {
                const float q = __expf(lg[e] - gmx) * ginv;
                const float d = q * (a.dq_ws[(int64_t)b * a.ld_dq + e] - qdq);
                const int64_t i = (int64_t)b * a.ld_dl + e;
                if (a.act_dtype == DMVAE_BF16) {
                    bf16_t* dl = reinterpret_cast<bf16_t*>(a.dlogits_act);
                    dl[i] = f2bf(bf2f(dl[i]) + d);
                } else {
                    float* dl = reinterpret_cast<float*>(a.dlogits_act);
                    dl[i] = dl[i] + d;
                }
            }
        }
        // featLearn: gmu[d] += sum_{e,o} dP[e,o] W[d, e O + o] * [mean_d > 0]
        if (a.featLearn && valid) {
            const float* mrow = a.mean + (int64_t)b * a.ld_mean;
            for (int d = 0; d < a.D; ++d) {
                const float* w = a.W + (int64_t)d * a.ldW;
                float acc = 0.f;
                for (int e = 0; e < E; ++e) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ov[j]) acc = fmaf(P[e * O + oo[j]], w[e * O + oo[j]], acc);
                }
                acc = row_sum16(acc);
                if (lane == (d & 15) && mrow[d] > 0.f) a.gmu[(int64_t)b * a.ld_g + d] += acc;
            }
        }
    }

    // per-workgroup partials: rows in ascending order
    __shared__ float red[MOE_ROWS][2];
    if (lane == 0) { red[grp][0] = valid ? loss : 0.f; red[grp][1] = valid ? err : 0.f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sl = 0.f, se = 0.f;
#pragma unroll
        for (int r = 0; r < MOE_ROWS; ++r) { sl += red[r][0]; se += red[r][1]; }
        float2 v; v.x = sl; v.y = se;
        reinterpret_cast<float2*>(a.partials)[blockIdx.x] = v;
    }
}

// sums the workgroup partials in a fixed order and updates the attachment's accumulators:
// acc[0] += inv_B * sum loss_b (loss_moe of the batch), acc[1] += error of the batch (classification: wrong rows;
// regression: inv_B * sum_b err_b), acc[2] = loss_moe of the batch, acc[3] = error of the batch
__global__ __launch_bounds__(256) void moe_finalize_kernel(const float* partials, int n, float inv_B, int classification, float* acc) {
    __shared__ float rl[256], re[256];
    float l = 0.f, e = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { l += partials[2 * i]; e += partials[2 * i + 1]; }
    rl[threadIdx.x] = l; re[threadIdx.x] = e;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { rl[threadIdx.x] += rl[threadIdx.x + s]; re[threadIdx.x] += re[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float loss = rl[0] * inv_B;
        const float err = classification ? re[0] : re[0] * inv_B;
        acc[0] += loss; acc[1] += err; acc[2] = loss; acc[3] = err;
    }
}

int moe_head_nblocks(int B_pad) { return (B_pad + MOE_ROWS - 1) / MOE_ROWS; }

#define MOE_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int moe_head_launch(hipStream_t s, const MoeHeadArgs& a) {
    MOE_REQUIRE(a.E >= 1 && a.E <= 256 && a.O >= 1 && a.O <= 64 && a.E * a.O <= 1024, "moe head: E=%d, O=%d (E <= 256, O <= 64, E*O <= 1024)", a.E, a.O);
    MOE_REQUIRE(a.P && a.logits && a.partials && (a.Y || a.B == 0), "moe head: null P / logits / partials / labels");
    MOE_REQUIRE(!a.backward || (a.dP_act && a.dlogits_act && a.dq_ws), "moe head: backward needs dP / dlogits / dq buffers");
    MOE_REQUIRE(!a.featLearn || (a.mean && a.W && a.bias && a.inp_act && (!a.backward || a.gmu)), "moe head: featLearn needs mean / W / bias / inp / gmu");
    const int nb = moe_head_nblocks(a.B_pad);
    DMVAE_LAUNCH(moe_head_kernel, dim3(nb), dim3(64), 0, s, a);
    {
        const int rc = check_launch("moe_head");
        if (rc) return rc;
    }
    DMVAE_LAUNCH(moe_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)a.partials, nb, a.inv_B, a.classification, a.acc);
    return check_launch("moe_finalize");
}

}  // namespace dmvae
