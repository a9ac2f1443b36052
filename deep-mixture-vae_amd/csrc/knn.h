// Exact k-nearest neighbours on the device (knn.hip): host-side launchers, and the distance tile body its all-pairs kernels share.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int KNN_MAX_N = 1 << 20;
constexpr int KNN_MAX_K = 256;
constexpr int KNN_MAX_C = 4096;
constexpr int KNN_ERR = 1;                       // err_flag bit: an index or a class out of range

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int64_t knn_ws_bytes(int64_t M, int64_t N, int D, int k);      // < 0: DMVAE_EINVAL
int knn_launch(hipStream_t s, const float* Q, int64_t ldq, int M, const float* X, int64_t ldx, int N, int D, int k, int64_t self_first, void* ws,
               int64_t ws_bytes, int32_t* idx, float* d2, int64_t ldo);
int knn_vote_launch(hipStream_t s, const int32_t* idx, int64_t ldi, int M, int k, const int32_t* classes, int N, int C, float* counts, int64_t ldc,
                    int32_t* err_flag);
int knn_ranks_launch(hipStream_t s, const float* X, int64_t ldx, int N, int D, const int32_t* idx, int64_t ldi, int k, int32_t* ranks, int64_t ldr,
                     int32_t* err_flag);

// ---- the distance tile: 16 query rows x 256 database columns (one per thread), the shape of sil_pairs_kernel --------------------------
constexpr int KNN_ROWS = 16, KNN_COLS = 256, KNN_DC = 32;
constexpr int KNN_LDJ = KNN_DC + 4;              // row stride of the column tile in LDS: 16-byte reads of 16 lanes fall into 64 distinct banks

struct KnnTile {
    __attribute__((aligned(16))) float xi[KNN_ROWS][KNN_DC];
    __attribute__((aligned(16))) float xj[KNN_COLS][KNN_LDJ];
};

// the key of the total order (d2, j): d2 >= +0 is finite or +inf, so its bit pattern orders as an unsigned integer
typedef unsigned long long knn_key_t;
constexpr knn_key_t KNN_KEY_MAX = ~0ull;         // (a NaN pattern: above every key of a real pair)
__device__ __forceinline__ knn_key_t knn_key(float d2, int j) { return ((knn_key_t)__float_as_uint(d2) << 32) | (unsigned)j; }

// acc[r] = d2(row i0 + r of Q, row j0 + threadIdx.x of X) for r < 16, by THE distance contract: acc = fmaf(q - x, q - x, acc) with f32
// differences, c ascending, acc starting at 0.  The rows pass through LDS KNN_DC columns at a time; rows >= M, columns >= N and the
// columns D .. of the last chunk are staged as zeros on both sides (fmaf(0, 0, acc) = acc).  All 256 threads call it; it begins every chunk
// with a barrier and ends without one.  xi_staged: D <= KNN_DC keeps the query tile staged for the whole walk of the workgroup.
__device__ __forceinline__ void knn_tile_d2(KnnTile& t, const float* __restrict__ Q, int64_t ldq, int M, int i0, const float* __restrict__ X, int64_t ldx,
                                            int N, int j0, int D, bool& xi_staged, float (&acc)[KNN_ROWS]) {
    const int tid = threadIdx.x;
    const int nchunk = (D + KNN_DC - 1) / KNN_DC;
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r) acc[r] = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int d0 = ch * KNN_DC;
        const int dn = D - d0 < KNN_DC ? D - d0 : KNN_DC;
        const int dn4 = (dn + 3) & ~3;
        __syncthreads();                                         // the previous chunk's (and the caller's) reads are done
        if (nchunk > 1 || !xi_staged) {
            for (int idx = tid; idx < KNN_ROWS * KNN_DC; idx += 256) {
                const int r = idx / KNN_DC, c = idx % KNN_DC;
                t.xi[r][c] = (i0 + r < M && c < dn) ? Q[(int64_t)(i0 + r) * ldq + d0 + c] : 0.f;
            }
            xi_staged = true;
        }
        // idx / dn4 for idx < 8192 and dn4 <= 32 by one multiply: the error of the reciprocal stays below 8192 / 2^20 < 1 / 32
        const unsigned inv = ((1u << 20) + dn4 - 1) / dn4;
        for (int idx = tid; idx < KNN_COLS * dn4; idx += 256) {
            const int r = (int)(((unsigned)idx * inv) >> 20), c = idx - r * dn4;
            t.xj[r][c] = (j0 + r < N && c < dn) ? X[(int64_t)(j0 + r) * ldx + d0 + c] : 0.f;
        }
        __syncthreads();
        for (int d = 0; d < dn4; d += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&t.xj[tid][d]);
#pragma unroll
            for (int r = 0; r < KNN_ROWS; ++r) {
                const float4 u = *reinterpret_cast<const float4*>(&t.xi[r][d]);
                const float e0 = u.x - v.x, e1 = u.y - v.y, e2 = u.z - v.z, e3 = u.w - v.w;
                acc[r] = fmaf(e0, e0, acc[r]);
                acc[r] = fmaf(e1, e1, acc[r]);
                acc[r] = fmaf(e2, e2, acc[r]);
                acc[r] = fmaf(e3, e3, acc[r]);
            }
        }
    }
}

}  // namespace dmvae
