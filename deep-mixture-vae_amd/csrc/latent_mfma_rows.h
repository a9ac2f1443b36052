// The row code the two MFMA forms of the latent stage share (latent_mfma.hip: DMVAE; latent_vade_mfma.hip: VaDE and its per-draw
// evaluation).  16 lanes per row; a lane owns quads of four columns.  Everything that follows a row through the stage exists here once:
// the quad loader, the reparameterisation of a quad, the Z / Z_f32 / clv stores, the wide-Z tail and the ones column, the sum of G2's
// K-slice slabs and the prior-table gradients from G3's batch slabs.  The loops around them (four quads per lane and trip in DMVAE's
// aligned paths, one in VaDE's) stay in the kernels.  Every function is inlined into its kernel: arguments that are constants there
// (no origin, no u half) cost nothing.
#pragma once
#include <algorithm>

#include "latent_tables.h"

namespace dmvae {

// every quad of every row of the stage's inputs and outputs can move as 16 bytes (the arrays themselves are 16-byte aligned: the plan's arena)
__device__ __forceinline__ bool latent_quads_aligned(const dmvae_latent_args& a) {
    return (a.D % 4 == 0) && (a.ld_mean % 4 == 0) && (a.ld_log_var % 4 == 0) && (a.ld_g % 4 == 0) && (a.ld_Z % 4 == 0) && (!a.eps || a.ld_eps % 4 == 0) &&
           (!a.Z_f32 || a.ld_Zf % 4 == 0);
}

// ---- mean, log_var and eps of the quad at column d0 of a row.  Unconditional loads with a clamped offset -- a load inside a divergent `if` is
// waited for at the join, a memory round trip each (DESIGN_LOG R4.2) -- so a pad quad reads quad 0, and the caller points a pad row at row 0; what
// they read is masked by reparam_quad.  vec: one 16-byte load per array (D % 4 == 0 and rows that keep 16-byte alignment: a quad is then
// inside the row or outside it).  erow == nullptr (device noise): ep = 0.
__device__ __forceinline__ void load_quad(const float* mrow, const float* vrow, const float* erow, bool vec, int d0, int D, float mu[4], float lv[4], float ep[4]) {
    if (vec) {
        const int off = d0 < D ? d0 : 0;
        const float4 m4 = *reinterpret_cast<const float4*>(mrow + off);
        const float4 l4 = *reinterpret_cast<const float4*>(vrow + off);
        const float4 e4 = erow ? *reinterpret_cast<const float4*>(erow + off) : make_float4(0.f, 0.f, 0.f, 0.f);
        mu[0] = m4.x; mu[1] = m4.y; mu[2] = m4.z; mu[3] = m4.w;
        lv[0] = l4.x; lv[1] = l4.y; lv[2] = l4.z; lv[3] = l4.w;
        ep[0] = e4.x; ep[1] = e4.y; ep[2] = e4.z; ep[3] = e4.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int off = d0 + j < D ? d0 + j : 0;
            mu[j] = mrow[off]; lv[j] = vrow[off];
            ep[j] = erow ? erow[off] : 0.f;
        }
    }
}

// ---- reparameterisation of one quad: z = mu + exp(lv / 2) ep, its coefficient cl = ep / 2 exp(lv / 2), the GEMM operand values
// x1 = e + mu^2 and mu (in place), lvsum += lv.  ok[j]: row and column are real (everything of a pad element is 0).  org (nullptr: none,
// DMVAE): the origin quad the operands are taken from (vade_origin_kernel) -- mu becomes mu - org before it is squared and zs = z - org; z itself
// is not shifted.  A caller that does not use an output does not pay for it.
__device__ __forceinline__ void reparam_quad(float mu[4], const float lv[4], const float ep[4], const bool ok[4], const float* org, float z[4], float cl[4],
                                             float x1[4], float zs[4], float& lvsum) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float e = __expf(lv[j]), sd = __expf(0.5f * lv[j]);
        z[j] = ok[j] ? mu[j] + sd * ep[j] : 0.f;
        cl[j] = ok[j] ? ep[j] * 0.5f * sd : 0.f;
        if (org) {
            mu[j] = ok[j] ? mu[j] - org[j] : 0.f;
            zs[j] = ok[j] ? z[j] - org[j] : 0.f;
        } else {
            mu[j] = ok[j] ? mu[j] : 0.f;
            zs[j] = z[j];
        }
        x1[j] = ok[j] ? e + mu[j] * mu[j] : 0.f;
        lvsum += ok[j] ? lv[j] : 0.f;
    }
}

// ---- outputs of one quad of row b: Z (act dtype; its pad columns up to ld_Z are written -- zeros -- because they are K padding of the first
// decoder GEMM), the f32 copy and the coefficient (columns < D).  vec: 8- / 16-byte stores while the quad is inside the Z row; element by element
// past ld_Z - 4 and for shapes that do not keep the alignment.
__device__ __forceinline__ void store_z_quad(const dmvae_latent_args& a, int64_t b, int d0, bool vec, const float z[4], const float cl[4]) {
    if (vec && d0 + 4 <= a.ld_Z) {
        if (a.act_dtype == DMVAE_BF16) {
            uint2 pk;
            pk.x = pack2bf(z[0], z[1]); pk.y = pack2bf(z[2], z[3]);
            *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.Z_act) + b * a.ld_Z + d0) = pk;
        } else *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.Z_act) + b * a.ld_Z + d0) = make_float4(z[0], z[1], z[2], z[3]);
        if (d0 < a.D) {
            if (a.Z_f32) *reinterpret_cast<float4*>(a.Z_f32 + b * a.ld_Zf + d0) = make_float4(z[0], z[1], z[2], z[3]);
            *reinterpret_cast<float4*>(a.clv + b * a.ld_g + d0) = make_float4(cl[0], cl[1], cl[2], cl[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = d0 + j;
            if (d < a.ld_Z) {
                if (a.act_dtype == DMVAE_BF16) reinterpret_cast<bf16_t*>(a.Z_act)[b * a.ld_Z + d] = f2bf(z[j]);
                else reinterpret_cast<float*>(a.Z_act)[b * a.ld_Z + d] = z[j];
            }
            if (d < a.D) {
                if (a.Z_f32) a.Z_f32[b * a.ld_Zf + d] = z[j];
                a.clv[b * a.ld_g + d] = cl[j];
            }
        }
    }
}

// columns [Dp, ld_Z) of row b of Z: zeros (a Z buffer wider than D padded to 64)
__device__ __forceinline__ void zero_z_tail(const dmvae_latent_args& a, int64_t b, int Dp, int lane16) {
    for (int d = Dp + lane16; d < a.ld_Z; d += 16) {
        if (a.act_dtype == DMVAE_BF16) reinterpret_cast<bf16_t*>(a.Z_act)[b * a.ld_Z + d] = 0;
        else reinterpret_cast<float*>(a.Z_act)[b * a.ld_Z + d] = 0.f;
    }
}

// the last 64 columns of an operand row [x1 | mu | 1]: the ones column (G3 then also yields the column sums of its other operand) and its padding
__device__ __forceinline__ void write_ones_column(float* ones, int lane16, bool valid) {
    for (int c = lane16; c < 64; c += 16) ones[c] = (c == 0 && valid) ? 1.f : 0.f;
}

// ---- the scores of N clusters of one row, summed over the slabs G2's K slices wrote (stride sstr), slabs in ascending order, in Acc.  The N loads
// of a slab are issued together.  QUAD: the clusters are off[0] .. off[0] + 3, read as 16 bytes.
template <typename Acc, int N, bool QUAD = false>
__device__ __forceinline__ void slab_sum(const float* S0, int64_t sstr, int nss, const int off[N], Acc v[N]) {
    static_assert(!QUAD || N == 4, "a quad is four clusters");
    float t[N];
    auto load = [&](int sl) {
        if constexpr (QUAD) {
            const float4 t4 = *reinterpret_cast<const float4*>(S0 + sl * sstr + off[0]);
            t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) t[j] = S0[sl * sstr + off[j]];
        }
    };
    load(0);
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (Acc)t[j];
    for (int sl = 1; sl < nss; ++sl) {
        load(sl);
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] += (Acc)t[j];
    }
}

// ---- the prior-table gradients from G3's slabs G[s][Kp][XW] = sums over batch slice s of w . [x1 | mu | 1]: what the workgroups >= first_wg of a
// *_post kernel do.  Slabs [0, ns): the weights' half (DMVAE's W, VaDE's gamma)
//     d pm = -r/B ip (G_mu - pm Wsum),   d plv = r/2B (Wsum - ip (G_e - 2 pm G_mu + pm^2 Wsum))
// U_HALF (VaDE): slabs [ns, 2 ns) hold du^T . [z^2 | z | 1], which adds  ip (Gu_z - pm Usum)  and  1/2 (ip (Gu_zz - 2 pm Gu_z + pm^2 Usum) - Usum).
// m0 (nullptr: 0): the origin the operands were taken from, pm - m0 here as in the tables.  Every sum over slabs in ascending order.
static inline int prior_grad_workgroups(int K, int D) { return (int)std::min<int64_t>(256, ((int64_t)K * D + 255) / 256); }      // the extra workgroups it gets
template <bool U_HALF>
__device__ __forceinline__ void prior_grad_from_slabs(const LatentWsHead& w, const float* ws, int64_t G, const float* prior_means, const float* m0, int K, int D, float rB,
                                                      float* dprior, int first_wg) {
    const int Dp = w.Dp, Kp = w.Kp, XW = w.XW, ns = w.nsplit;
    const float rB2 = 0.5f * rB;
    const int64_t KD = (int64_t)K * D;
    for (int64_t idx = (int64_t)((int)blockIdx.x - first_wg) * 256 + threadIdx.x; idx < KD; idx += (int64_t)((int)gridDim.x - first_wg) * 256) {
        const int k = (int)(idx / D), d = (int)(idx - (int64_t)k * D);
        float ge = 0.f, gm = 0.f, wsum = 0.f, gzz = 0.f, gz = 0.f, usum = 0.f;
        for (int s = 0; s < ns; ++s) {
            const float* g = ws + G + ((int64_t)s * Kp + k) * XW;
            ge += g[d]; gm += g[Dp + d]; wsum += g[2 * Dp];
        }
        if constexpr (U_HALF)
            for (int s = ns; s < 2 * ns; ++s) {
                const float* g = ws + G + ((int64_t)s * Kp + k) * XW;
                gzz += g[d]; gz += g[Dp + d]; usum += g[2 * Dp];
            }
        const float ip = ws[w.T1 + (int64_t)k * 2 * Dp + d];
        const float pmv = m0 ? prior_means[idx] - m0[d] : prior_means[idx];
        float dm = -rB * ip * (gm - pmv * wsum);
        float dv = rB2 * (wsum - ip * (ge - 2.f * pmv * gm + pmv * pmv * wsum));
        if constexpr (U_HALF) {
            dm = dm + ip * (gz - pmv * usum);
            dv = dv + 0.5f * (ip * (gzz - 2.f * pmv * gz + pmv * pmv * usum) - usum);
        }
        dprior[idx] = dm;
        dprior[KD + idx] = dv;
    }
}

}  // namespace dmvae
