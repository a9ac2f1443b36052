// What the two MFMA forms of the latent stage share on the host side and around their GEMMs (latent_mfma.hip: DMVAE; latent_vade_mfma.hip:
// VaDE): the head of the scratch layout and its slice-count rule, the prior tables as GEMM operands, the description of one exact-f32
// STORE_F32 problem and the profiled launch of a row kernel.  The row code of their kernels: latent_mfma_rows.h.
#pragma once
#include <string.h>

#include "kernels.h"

namespace dmvae {

static inline int pad64i(int x) { return (x + 63) / 64 * 64; }

// ---- scratch layout (float offsets into the caller's scratch).  Both forms start with the table operands; each goes on with its own arrays.
struct LatentWsHead {
    int Dp, Kp, XW, nsplit, nsplit_s;      // K slices of (each half of) G3 (over the batch) and of G2 (over 2D)
    int64_t T1, T2, c2, ck;
};
struct WsTake {                            // the next n floats, every array starting on a multiple of 64
    int64_t o = 0;
    int64_t operator()(int64_t n) { const int64_t r = o; o += (n + 63) / 64 * 64; return r; }
};
// K slices of a GEMM whose one-slice grid is `tiles * rowf` workgroups: doubled while the grid stays under 512 workgroups (fill the chip), up to
// `cap`, and while the `units` 64-wide steps of the contraction still split evenly
static inline int latent_slice_count(int tiles, int rowf, int cap, int units) {
    int n = 1;
    while (n < cap && tiles * rowf * n < 512 && units % (2 * n) == 0) n *= 2;
    return n;
}
// rowf: stacked row blocks of the operands (DMVAE 1; VaDE 2: mean rows, then sample rows).  G3 contracts over the batch (per half), in multiples
// of 64 rows.  G2 = [rowf B, 2D] x [2D, K]: with few rows and clusters its grid is a handful of workgroups of a long K loop -- cut 2D, up to cap_s
// slices.  (VaDE: shorter fmaf chains are also what keeps u accurate at D = 512; a full chip takes the one-slice form.)
static inline WsTake latent_ws_head(LatentWsHead& w, int Bp, int D, int K, int rowf, int cap_s) {
    w.Dp = pad64i(D); w.Kp = pad64i(K); w.XW = 2 * w.Dp + 64;
    w.nsplit = latent_slice_count((w.Kp / 64) * (w.XW / 64), rowf, 32, Bp / 64);
    w.nsplit_s = latent_slice_count((Bp / 64) * (w.Kp / 64), rowf, cap_s, 2 * w.Dp / 64);
    WsTake take;
    w.T1 = take((int64_t)w.Kp * 2 * w.Dp); w.T2 = take((int64_t)w.Kp * 2 * w.Dp);
    w.c2 = take(w.Kp); w.ck = take(w.Kp);
    return take;
}

// ---- prior tables -> GEMM operands (tiny: K * D elements)
//   T1 = [ip | pm ip],  T2 = [ip | -2 pm ip]  ([Kp][2 Dp], pad rows / columns zero),  c2_k = sum_d pm^2 ip,  ck_k = sum_d plv
//   m0 (nullptr: none): the origin [Dp] the means are taken from, pm - m0 in every product (latent_vade_mfma.hip: vade_origin_kernel)
__device__ __forceinline__ void latent_tables_block(const int k, const float* __restrict__ pm, const float* __restrict__ plv, const float* __restrict__ m0, int K, int D,
                                                    const LatentWsHead& w, float* __restrict__ ws, float* red) {
    // one block per (padded) cluster row k
    const int Dp = w.Dp;
    float* T1 = ws + w.T1 + (int64_t)k * 2 * Dp;
    float* T2 = ws + w.T2 + (int64_t)k * 2 * Dp;
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
        T1[d] = ip;
        T1[Dp + d] = m * ip;
        T2[d] = ip;
        T2[Dp + d] = -2.f * m * ip;
    }
    const float a = block_sum_256(s2, red);
    const float b = block_sum_256(sl, red + 4);
    if (threadIdx.x == 0) { ws[w.c2 + k] = a; ws[w.ck + k] = b; }
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

// one launch of a 256-thread kernel of the stage under its profiling scope (closed before the launch is checked)
template <typename... P, typename... A>
static inline int latent_launch_rows(hipStream_t s, const char* name, double bytes, void (*kernel)(P...), int grid, A... args) {
    {
        ProfScope ps(s, name, 0.0, bytes);
        DMVAE_LAUNCH(kernel, dim3(grid), dim3(256), 0, s, args...);
    }
    return check_launch(name);
}

}  // namespace dmvae
