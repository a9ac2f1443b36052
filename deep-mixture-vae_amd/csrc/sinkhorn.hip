// The softmin pass of the log-domain Sinkhorn iteration on the device: for rows X [N][ldx] against columns Y [M][ldy], all pairs, no N x M
// array stored,
//   h_j = log_b_j + g_j / eps        t_ij = h_j - d2(i, j) / eps        out_i = -eps logsumexp_j t_ij        (or (prev_i + that) / 2)
// with d2 THE distance contract of knn.hip -- acc = fmaf(x_c - y_c, x_c - y_c, acc), f32 differences, c ascending -- from the SAME tile body
// (knn_tile_d2 of knn.h), so a pair's bits are those dmvae_knn returns.  Both half-steps of a Sinkhorn iteration are this kernel with the
// roles of X and Y swapped; the symmetric problems pass the same rows twice and their potential as prev.
//   sinkhorn_softmin_kernel  a workgroup owns 16 rows and walks all the columns in tiles of 256, one per thread.  A thread forms its column's
//                            h_j = fmaf(g_j, 1 / eps, log_b_j) once per tile (-inf past the last column), after the tile the 16 values
//                            t = fmaf(-d2, 1 / eps, h), and pushes each into a per-row running logsumexp kept in registers across the walk:
//                            (max f32, scaled sum f64), MdLse of lse.h as in mixture_density.hip -- one __expf per pair, the sum in double, so that the
//                            number of tiles does not enter the error.  The 256 partials of a row are joined ONCE, at the end, in a fixed order:
//                            an xor butterfly whose join (md_join) is symmetric in its arguments, then the four waves ascending through LDS.  16 threads
//                            finish: -eps (m + log s) in double, averaged with prev there, rounded once.  A column with h_j = -inf never
//                            enters; a row whose columns are all empty gets +inf.  No NaN is formed from finite inputs.
// No float atomics, no spinning, every loop bounded by the arguments: two calls on the same inputs return the same bits.  One launch, no
// workspace, no split for few rows (both sets hold thousands of rows in every use, as prdc_pairs_kernel).
#include <math.h>

#include "sinkhorn.h"
#include "knn.h"
#include "lse.h"

namespace dmvae {

struct SinkhornArgs {
    const float* X; int64_t ldx; int N;
    const float* Y; int64_t ldy; int M;
    int D;
    const float* g; const float* log_b; const float* prev;
    float eps, inv_eps, log_b_uniform;           // 1 / eps rounded once on the host; -log M where log_b is null
    float* out;
};

__global__ __launch_bounds__(256) void sinkhorn_softmin_kernel(SinkhornArgs a) {
    __shared__ KnnTile tile;
    __shared__ float redm[4][KNN_ROWS];                          // per wave: a row's joined pair
    __shared__ double reds[4][KNN_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i0 = blockIdx.x * KNN_ROWS;
    const int N = a.N, M = a.M;
    const float inv_eps = a.inv_eps;
    float m[KNN_ROWS];
    double s[KNN_ROWS];
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r) { m[r] = -INFINITY; s[r] = 0.0; }
    bool xi_staged = false;
    float acc[KNN_ROWS];

    for (int j0 = 0; j0 < M; j0 += KNN_COLS) {
        const int j = j0 + tid;
        float h = -INFINITY;                                     // the ragged last tile: its columns (staged as zeros) never enter
        if (j < M) {
            const float lb = a.log_b ? a.log_b[j] : a.log_b_uniform;
            h = a.g ? fmaf(a.g[j], inv_eps, lb) : lb;
        }
        knn_tile_d2(tile, a.X, a.ldx, N, i0, a.Y, a.ldy, M, j0, a.D, xi_staged, acc);
#pragma unroll
        for (int r = 0; r < KNN_ROWS; ++r) {
            const float x = fmaf(-acc[r], inv_eps, h);           // -inf for an empty column and for a d2 that overflowed; a NaN fails both tests below
            const double e = (double)__expf(-fabsf(x - m[r]));   // (unused where x = m = -inf makes it a NaN)
            const bool up = x > m[r];
            s[r] = up ? fma(s[r], e, 1.0) : (x > -INFINITY ? s[r] + e : s[r]);
            m[r] = up ? x : m[r];
        }
    }

    // the 256 pairs of every row, in a fixed order
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r) {
        MdLse v{m[r], s[r]};
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = md_join(v, MdLse{__shfl_xor(v.m, o, 64), __shfl_xor(v.s, o, 64)});
        if (lane == 0) { redm[w][r] = v.m; reds[w][r] = v.s; }
    }
    __syncthreads();
    if (tid < KNN_ROWS && i0 + tid < N) {
        MdLse v{redm[0][tid], reds[0][tid]};
#pragma unroll
        for (int k = 1; k < 4; ++k) v = md_join(v, MdLse{redm[k][tid], reds[k][tid]});
        const int64_t i = (int64_t)i0 + tid;
        double o = v.s > 0.0 ? -(double)a.eps * ((double)v.m + log(v.s)) : (double)INFINITY;
        if (a.prev) o = 0.5 * ((double)a.prev[i] + o);
        a.out[i] = (float)o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define SINKHORN_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int sinkhorn_softmin_launch(hipStream_t s, const float* X, int64_t ldx, int N, const float* Y, int64_t ldy, int M, int D, const float* g, const float* log_b,
                            float eps, const float* prev, float* out) {
    const char* who = "dmvae_sinkhorn_softmin";
    SINKHORN_REQUIRE(N >= 1 && N <= KNN_MAX_N && M >= 1 && M <= KNN_MAX_N, "%s: N=%d, M=%d (1 .. %d)", who, N, M, KNN_MAX_N);
    SINKHORN_REQUIRE(D >= 1, "%s: D=%d (D >= 1)", who, D);
    SINKHORN_REQUIRE(X && Y && out, "%s: null X / Y / out", who);
    SINKHORN_REQUIRE(ldx >= D && ldy >= D, "%s: ldx=%lld, ldy=%lld (ldx >= D, ldy >= D)", who, (long long)ldx, (long long)ldy);
    SINKHORN_REQUIRE(isfinite(eps) && eps > 0.f && isfinite(1.0f / eps), "%s: eps=%g (finite, > 0, 1 / eps finite in f32)", who, (double)eps);
    const double groups = (double)((N + KNN_ROWS - 1) / KNN_ROWS);
    // per pair: a subtraction and an fma per column, then the fma of t, the difference, the exponential, the conversion and the f64 update
    ProfScope ps(s, "sinkhorn_softmin", (double)N * M * (3.0 * D + 8.0), 4.0 * M * ((D + (g ? 1.0 : 0.0) + (log_b ? 1.0 : 0.0)) * groups) +
                                                                             4.0 * N * (D + 1.0 + (prev ? 1.0 : 0.0)));
    const SinkhornArgs a{X, ldx, N, Y, ldy, M, D, g, log_b, prev, eps, 1.0f / eps, (float)-log((double)M), out};
    DMVAE_LAUNCH(sinkhorn_softmin_kernel, dim3((N + KNN_ROWS - 1) / KNN_ROWS), dim3(256), 0, s, a);
    return check_launch(who);
}

}  // namespace dmvae
