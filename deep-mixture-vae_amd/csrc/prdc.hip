// Sample quality on the device: the counts behind improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage
// (Naeem et al. 2020) of generated rows F [M][ldf] against real rows R [N][ldr], all pairs, no N x M array stored.  One distance,
//   d2(i, j) = acc after  acc = fmaf(r_ic - f_jc, r_ic - f_jc, acc)  over c ascending, f32 differences, acc starting at 0
// -- the distance contract of knn.hip, taken from the SAME tile body (knn_tile_d2 of knn.h), so a pair's bits are those dmvae_knn returns
// and a radius it returned is met exactly.  Negating an f32 difference is exact: d2(R_i, F_j) and d2(F_j, R_i) are the same bits, and ONE
// pass over the pairs serves both directions.  Radii are SQUARED distances and inputs (no k, no square root); balls are CLOSED: d2 <= r2.
//   prdc_pairs_kernel  a workgroup owns 16 real rows and walks all the generated rows in tiles of 256 columns, one per thread.  After a
//                      tile a thread holds the 16 d2 of its column j.  Per real row it keeps, in registers across the walk, the smallest
//                      key (d2, j) (knn_key: an unsigned integer minimum, order-free, the lowest j on a tie) and the number of its
//                      columns with d2 <= rF2[j]; both are joined across the 256 threads ONCE, at the end of the walk: wave shuffles,
//                      then 4 partials per row through LDS.  Per column it counts the workgroup's rows with d2 <= rR2[i] and, where that
//                      is not zero, adds it to fake_in_real[j] with one INTEGER atomic: integer addition commutes, the result is the same
//                      bits on every call.  Rows >= N and columns >= M (staged as zeros by the tile) count nowhere.
// No float atomics, no sum of floats outside the distance itself.
#include "prdc.h"
#include "knn.h"

namespace dmvae {

struct PrdcArgs {
    const float* R; int64_t ldr; int N;
    const float* F; int64_t ldf; int M;
    int D;
    const float* rR2; const float* rF2;
    int32_t* fake_in_real; int32_t* real_in_fake; float* real_min_d2; int32_t* real_min_j;
};

__device__ __forceinline__ knn_key_t prdc_wave_min(knn_key_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const knn_key_t other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}
__device__ __forceinline__ int prdc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void prdc_pairs_kernel(PrdcArgs a) {
    __shared__ KnnTile tile;
    __shared__ float rr[KNN_ROWS];                               // the squared radii of the workgroup's real rows
    __shared__ knn_key_t wmin[4][KNN_ROWS];                      // per wave: a row's smallest key, its count
    __shared__ int wcnt[4][KNN_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i0 = blockIdx.x * KNN_ROWS;
    const int N = a.N, M = a.M;
    const int nrows = N - i0 < KNN_ROWS ? N - i0 : KNN_ROWS;     // >= 1: the grid is ceil(N / 16)
    if (tid < KNN_ROWS) rr[tid] = tid < nrows ? a.rR2[i0 + tid] : 0.f;
    knn_key_t best[KNN_ROWS];
    int cnt[KNN_ROWS];
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r) { best[r] = KNN_KEY_MAX; cnt[r] = 0; }
    bool xi_staged = false;
    float acc[KNN_ROWS];

    for (int j0 = 0; j0 < M; j0 += KNN_COLS) {
        const int j = j0 + tid;
        knn_tile_d2(tile, a.R, a.ldr, N, i0, a.F, a.ldf, M, j0, a.D, xi_staged, acc);          // (its first barrier publishes rr)
        if (j < M) {
            const float rf = a.rF2[j];
            int col = 0;
#pragma unroll
            for (int r = 0; r < KNN_ROWS; ++r) {
                if (r < nrows) {
                    const knn_key_t key = knn_key(acc[r], j);
                    best[r] = key < best[r] ? key : best[r];
                    cnt[r] += acc[r] <= rf;
                    col += acc[r] <= rr[r];
                }
            }
            if (col) atomicAdd(&a.fake_in_real[j], col);
        }
    }
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r) {
        const knn_key_t m = prdc_wave_min(best[r]);
        const int c = prdc_wave_sum(cnt[r]);
        if (lane == 0) { wmin[w][r] = m; wcnt[w][r] = c; }
    }
    __syncthreads();
    if (tid < nrows) {
        knn_key_t m = wmin[0][tid];
        int c = wcnt[0][tid];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            m = wmin[q][tid] < m ? wmin[q][tid] : m;
            c += wcnt[q][tid];
        }
        const int64_t i = (int64_t)i0 + tid;
        a.real_in_fake[i] = c;
        a.real_min_d2[i] = __uint_as_float((unsigned)(m >> 32));
        if (a.real_min_j) a.real_min_j[i] = (int32_t)(unsigned)m;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define PRDC_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int prdc_counts_launch(hipStream_t s, const float* R, int64_t ldr, int N, const float* F, int64_t ldf, int M, int D, const float* rR2, const float* rF2,
                       int32_t* fake_in_real, int32_t* real_in_fake, float* real_min_d2, int32_t* real_min_j) {
    const char* who = "dmvae_prdc_counts";
    PRDC_REQUIRE(N >= 1 && N <= KNN_MAX_N && M >= 1 && M <= KNN_MAX_N, "%s: N=%d, M=%d (1 .. %d)", who, N, M, KNN_MAX_N);
    PRDC_REQUIRE(D >= 1, "%s: D=%d (D >= 1)", who, D);
    PRDC_REQUIRE(R && F && rR2 && rF2, "%s: null R / F / rR2 / rF2", who);
    PRDC_REQUIRE(fake_in_real && real_in_fake && real_min_d2, "%s: null fake_in_real / real_in_fake / real_min_d2", who);
    PRDC_REQUIRE(ldr >= D && ldf >= D, "%s: ldr=%lld, ldf=%lld (ldr >= D, ldf >= D)", who, (long long)ldr, (long long)ldf);
    ProfScope ps(s, "prdc_counts", (double)N * M * (3.0 * D + 6.0), 4.0 * M * ((double)(D + 1) * ((N + KNN_ROWS - 1) / KNN_ROWS)) + 4.0 * N * (D + 4.0));
    if (hipError_t e = hipMemsetAsync(fake_in_real, 0, (size_t)M * sizeof(int32_t), s)) {
        set_error("%s: clearing fake_in_real: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    const PrdcArgs a{R, ldr, N, F, ldf, M, D, rR2, rF2, fake_in_real, real_in_fake, real_min_d2, real_min_j};
    DMVAE_LAUNCH(prdc_pairs_kernel, dim3((N + KNN_ROWS - 1) / KNN_ROWS), dim3(256), 0, s, a);
    return check_launch(who);
}

}  // namespace dmvae
