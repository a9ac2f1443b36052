// What the two MFMA forms of the latent stage share (latent_mfma.hip: DMVAE; latent_vade_mfma.hip: VaDE): the prior tables as
// GEMM operands and the description of one exact-f32 STORE_F32 problem.
#pragma once
#include <string.h>

#include "kernels.h"

namespace dmvae {

static inline int pad64i(int x) { return (x + 63) / 64 * 64; }

// ---- prior tables -> GEMM operands (tiny: K * D elements)
//   T1 = [ip | pm ip],  T2 = [ip | -2 pm ip]  ([Kp][2 Dp], pad rows / columns zero),  c2_k = sum_d pm^2 ip,  ck_k = sum_d plv
//   m0 (nullptr: none): the origin [Dp] the means are taken from, pm - m0 in every product (latent_vade_mfma.hip: vade_origin_kernel)
__device__ __forceinline__ void latent_tables_block(const int k, const float* __restrict__ pm, const float* __restrict__ plv, const float* __restrict__ m0, int K, int D, int Kp, int Dp,
                                                    float* __restrict__ T1, float* __restrict__ T2, float* __restrict__ c2, float* __restrict__ ck, float* red) {
    // one block per (padded) cluster row k
    float s2 = 0.f, sl = 0.f;
    for (int d = threadIdx.x; d < Dp; d += 256) {
        float ip = 0.f, m = 0.f;
        if (k < K && d < D) {
            const float lv = plv[(int64_t)k * D + d];
            m = pm[(int64_t)k * D + d];
            if (m0) m -= m0[d];
            ip = __expf(-lv);
            s2 += m * m * ip;
            sl += lv;
        }
        T1[(int64_t)k * 2 * Dp + d] = ip;
        T1[(int64_t)k * 2 * Dp + Dp + d] = m * ip;
        T2[(int64_t)k * 2 * Dp + d] = ip;
        T2[(int64_t)k * 2 * Dp + Dp + d] = -2.f * m * ip;
    }
    const float a = block_sum_256(s2, red);
    const float b = block_sum_256(sl, red + 4);
    if (threadIdx.x == 0) { c2[k] = a; ck[k] = b; }
}

static inline GemmArgs f32_problem(int M, int N, int K, const float* A, int64_t lda, const float* B, int64_t ldb, float* out, int64_t ldo,
                                   int split, int64_t slab_stride) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.k_split = K / split; g.group_m = 8; g.conv_p = 0; g.conv_c = 0;
    memset(&g.epi, 0, sizeof(g.epi));
    g.epi.kind = DMVAE_EPI_STORE_F32; g.epi.out = out; g.epi.ldo = ldo; g.epi.m_valid = M; g.epi.n_valid = N;
    g.slab_stride = slab_stride;
    return g;
}

}  // namespace dmvae
