// Exact k-nearest neighbours in latent space on the device: the k rows of X [N][ldx] nearest every row of Q [M][ldq] under
//   d2(i, j) = acc after  acc = fmaf(q_ic - x_jc, q_ic - x_jc, acc)  over c ascending, f32 differences, acc starting at 0
// (no norm expansion: near rows do not cancel -- cluster_metrics.hip), ordered by the TOTAL order (d2, j) ascending: an exact tie goes to the
// lower row.  A pair is one 64-bit key, (bits of d2) << 32 | j: d2 >= +0, so the keys order as unsigned integers exactly as the pairs do, no
// two keys of one query are equal, and the k smallest are ONE set whatever order the candidates arrive in.  No N x M array is stored.
//   knn_pairs_kernel   a workgroup owns 16 query rows and walks its share of the database in tiles of 256 columns, one per thread
//                      (knn_tile_d2 of knn.h, the tile of sil_pairs_kernel).  Per query row LDS keeps L = k + cap keys: the sorted best k,
//                      behind them a candidate buffer, and beside them the threshold (the k-th key; all ones until k are held) and the
//                      buffer's fill.  A thread whose column lies below a row's threshold appends its key (one LDS integer atomic for the
//                      slot).  A row whose buffer is full is sorted by one wave -- a bitonic network over keys in LDS, every comparator
//                      ascending, so a length that is no power of two needs no padding -- which lowers the threshold; the candidates that
//                      found no slot are compared against the new threshold and try again.  With random rows a query sees about
//                      k (1 + ln(N / k)) insertions out of N columns.
//   knn_merge_kernel   few queries against many rows (the exemplars of K prior means): the database is dealt to S workgroups per query
//                      tile, each leaves its k best keys in the workspace, and one wave per query sorts the S k keys.  The k smallest keys
//                      of the whole are among the k smallest of every part, so S changes no bit of the result.
//   knn_vote_kernel    one workgroup per query: an integer histogram of its neighbours' classes in LDS, written out as f32 counts
//   knn_ranks_kernel   ranks[i][t] = #{l != i: (d2(i, l), l) < (d2(i, j), j)}, j = idx[i][t]: the 16 x k keys of a workgroup's rows sit in LDS,
//                      the same tile walk leaves the 16 x 256 keys of a column tile beside them, and every thread counts the tile's keys
//                      below the thresholds it owns (no atomics: a counter has one owner)
// No float atomics, no sum of floats outside the distance itself: two calls on the same inputs return the same bits.
#include "knn.h"

namespace dmvae {

constexpr int KNN_MAX_SPLIT = 16;
constexpr int KNN_CKLD = KNN_COLS + 1;           // row stride of the ranks kernel's column keys: rows fall into different banks

static int knn_list_len(int k) { return (k + 32 + 63) / 64 * 64; }       // L: the best k and a buffer of 32 .. 95 candidates
static size_t knn_pairs_lds(int L) { return (size_t)KNN_ROWS * ((size_t)L * sizeof(knn_key_t) + sizeof(knn_key_t) + sizeof(int)); }
__host__ __device__ static inline int knn_pow2(int v) { int p = 2; while (p < v) p <<= 1; return p; }

// keys row[0 .. L) ascending, by one wave: the bitonic network on P = 2^n >= L positions in the form whose comparators all put the smaller
// key at the lower position (first step of a stage against the mirrored partner).  The positions L .. P hold nothing: they stand for
// +infinity behind every real key, which no comparator would move, so a comparator that reaches one is skipped.  Same wave, in-order LDS.
__device__ __forceinline__ void knn_cmpx(knn_key_t* row, int i, int l, int L) {
    if (l < L) {
        const knn_key_t a = row[i], b = row[l];
        if (b < a) { row[i] = b; row[l] = a; }
    }
}
__device__ void knn_sort_row(knn_key_t* row, int L, int P, int lane) {
    for (int lh = 0; (2 << lh) <= P; ++lh) {                     // stage: runs of 2 << lh
        const int half = 1 << lh;
        for (int t = lane; t < (P >> 1); t += 64) {
            const int i = ((t >> lh) << (lh + 1)) + (t & (half - 1));
            knn_cmpx(row, i, i ^ ((half << 1) - 1), L);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int ls = lh - 1; ls >= 0; --ls) {
            const int stride = 1 << ls;
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t >> ls) << (ls + 1)) + (t & (stride - 1));
                knn_cmpx(row, i, i + stride, L);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
}

struct KnnArgs {
    const float* Q; int64_t ldq; int M;
    const float* X; int64_t ldx; int N, D, k;
    int64_t self_first;
    int L, tiles_per_split, nsplit;
    knn_key_t* part;                             // [nsplit][M][k], or null: nsplit = 1 writes idx / d2
    int32_t* idx; float* d2; int64_t ldo;
};

__global__ __launch_bounds__(256) void knn_pairs_kernel(KnnArgs a) {
    __shared__ KnnTile tile;
    extern __shared__ __attribute__((aligned(16))) knn_key_t sel[];          // [16][L], then thr [16] and cnt [16] (knn_pairs_lds)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i0 = blockIdx.x * KNN_ROWS;
    const int k = a.k, L = a.L, cap = L - k, N = a.N;
    knn_key_t* thr = sel + KNN_ROWS * L;                         // the k-th key of a row's list
    int* cnt = (int*)(thr + KNN_ROWS);                           // candidates appended since the row's last sort (may run past cap)
    for (int e = tid; e < KNN_ROWS * L; e += 256) sel[e] = KNN_KEY_MAX;
    if (tid < KNN_ROWS) { thr[tid] = KNN_KEY_MAX; cnt[tid] = 0; }
    const int ntiles = (N + KNN_COLS - 1) / KNN_COLS;
    const int t_lo = blockIdx.y * a.tiles_per_split;
    const int t_hi = t_lo + a.tiles_per_split < ntiles ? t_lo + a.tiles_per_split : ntiles;
    bool xi_staged = false;
    float acc[KNN_ROWS];

    for (int tl = t_lo; tl < t_hi; ++tl) {
        const int j0 = tl * KNN_COLS, j = j0 + tid;
        knn_tile_d2(tile, a.Q, a.ldq, a.M, i0, a.X, a.ldx, N, j0, a.D, xi_staged, acc);         // (its first barrier publishes thr / cnt / sel)
        unsigned pending = 0;
        if (j < N) {
#pragma unroll
            for (int r = 0; r < KNN_ROWS; ++r) {
                const bool self = a.self_first >= 0 && a.self_first + i0 + r == (int64_t)j;
                if (i0 + r < a.M && !self && knn_key(acc[r], j) < thr[r]) pending |= 1u << r;
            }
        }
        while (__syncthreads_or(pending != 0)) {                 // (every thread has read the thresholds it needs)
#pragma unroll
            for (int r = 0; r < KNN_ROWS; ++r) {
                if (pending >> r & 1) {
                    const int pos = atomicAdd(&cnt[r], 1);
                    if (pos < cap) { sel[r * L + k + pos] = knn_key(acc[r], j); pending &= ~(1u << r); }
                }
            }
            __syncthreads();
            for (int r = w; r < KNN_ROWS; r += 4) {              // a full row: sort, lower the threshold, empty the buffer
                if (cnt[r] >= cap) {                             // (the whole wave)
                    knn_sort_row(sel + r * L, L, knn_pow2(L), lane);
                    if (lane == 0) { thr[r] = sel[r * L + k - 1]; cnt[r] = 0; }
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < KNN_ROWS; ++r)
                if ((pending >> r & 1) && !(knn_key(acc[r], j) < thr[r])) pending &= ~(1u << r);
        }
    }
    __syncthreads();
    for (int r = w; r < KNN_ROWS; r += 4) {                      // what the buffers still hold
        const int n = cnt[r] < cap ? cnt[r] : cap;
        if (n > 0) knn_sort_row(sel + r * L, k + n, knn_pow2(k + n), lane);
    }
    __syncthreads();
    for (int e = tid; e < KNN_ROWS * k; e += 256) {
        const int r = e / k, t = e - r * k;
        if (i0 + r >= a.M) break;
        const knn_key_t key = sel[r * L + t];
        if (a.part) {
            a.part[((int64_t)blockIdx.y * a.M + i0 + r) * k + t] = key;
        } else {
            a.idx[(int64_t)(i0 + r) * a.ldo + t] = (int32_t)(unsigned)key;
            a.d2[(int64_t)(i0 + r) * a.ldo + t] = __uint_as_float((unsigned)(key >> 32));
        }
    }
}

__global__ __launch_bounds__(64) void knn_merge_kernel(const knn_key_t* __restrict__ part, int M, int k, int nsplit, int32_t* __restrict__ idx,
                                                       float* __restrict__ d2, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) knn_key_t keys[];         // [nsplit][k]
    const int i = blockIdx.x, lane = threadIdx.x, n = nsplit * k;
    for (int e = lane; e < n; e += 64) keys[e] = part[((int64_t)(e / k) * M + i) * k + e % k];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    knn_sort_row(keys, n, knn_pow2(n), lane);
    for (int t = lane; t < k; t += 64) {
        idx[(int64_t)i * ldo + t] = (int32_t)(unsigned)keys[t];
        d2[(int64_t)i * ldo + t] = __uint_as_float((unsigned)(keys[t] >> 32));
    }
}

__global__ __launch_bounds__(256) void knn_vote_kernel(const int32_t* __restrict__ idx, int64_t ldi, int k, const int32_t* __restrict__ classes, int N,
                                                       int C, float* __restrict__ counts, int64_t ldc, int32_t* err_flag) {
    __shared__ int hist[KNN_MAX_C];
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) hist[c] = 0;
    __syncthreads();
    for (int t = tid; t < k; t += 256) {
        const int j = idx[(int64_t)i * ldi + t];
        if (j < 0 || j >= N) { atomicOr(err_flag, KNN_ERR); continue; }      // checked before it indexes anything
        const int c = classes[j];
        if (c < 0 || c >= C) { atomicOr(err_flag, KNN_ERR); continue; }
        atomicAdd(&hist[c], 1);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) counts[(int64_t)i * ldc + c] = (float)hist[c];
}

struct KnnRankArgs {
    const float* X; int64_t ldx; int N, D;
    const int32_t* idx; int64_t ldi; int k;
    int32_t* ranks; int64_t ldr; int32_t* err_flag;
};

__global__ __launch_bounds__(256) void knn_ranks_kernel(KnnRankArgs a) {
    __shared__ KnnTile tile;
    extern __shared__ __attribute__((aligned(16))) knn_key_t dyn[];
    const int tid = threadIdx.x, i0 = blockIdx.x * KNN_ROWS, k = a.k, N = a.N, D = a.D, npair = KNN_ROWS * k;
    knn_key_t* thrk = dyn;                                       // [16][k] the key of (i, idx[i][t]); 0 (below which no key lies) where refused
    knn_key_t* ckey = dyn + npair;                               // [16][KNN_CKLD] the keys of the column tile
    int* below = (int*)(ckey + KNN_ROWS * KNN_CKLD);             // [16][k] keys counted below; -1: a refused pair (0 is a real key: row 0 at d2 = 0)
    for (int e = tid; e < npair; e += 256) {
        const int r = e / k, t = e - r * k, i = i0 + r;
        knn_key_t key = 0;
        int start = -1;
        if (i < N) {
            const int j = a.idx[(int64_t)i * a.ldi + t];
            if (j < 0 || j >= N || j == i) {
                atomicOr(a.err_flag, KNN_ERR);                   // checked before it indexes anything
            } else {
                const float* xi = a.X + (int64_t)i * a.ldx;
                const float* xj = a.X + (int64_t)j * a.ldx;
                float acc = 0.f;
                for (int c = 0; c < D; ++c) {
                    const float e0 = xi[c] - xj[c];
                    acc = fmaf(e0, e0, acc);
                }
                key = knn_key(acc, j);
                start = 0;
            }
        }
        thrk[e] = key;
        below[e] = start;
    }
    bool xi_staged = false;
    float acc[KNN_ROWS];
    for (int j0 = 0; j0 < N; j0 += KNN_COLS) {
        const int j = j0 + tid;
        knn_tile_d2(tile, a.X, a.ldx, N, i0, a.X, a.ldx, N, j0, D, xi_staged, acc);  // (its first barrier ends the previous tile's counting)
#pragma unroll
        for (int r = 0; r < KNN_ROWS; ++r) ckey[r * KNN_CKLD + tid] = (j < N && j != i0 + r) ? knn_key(acc[r], j) : KNN_KEY_MAX;
        __syncthreads();
        for (int e = tid; e < npair; e += 256) {
            const knn_key_t th = thrk[e];
            const knn_key_t* col = ckey + (e / k) * KNN_CKLD;
            int c = 0;
            for (int q = 0; q < KNN_COLS; ++q) c += col[q] < th;
            below[e] += c;
        }
    }
    for (int e = tid; e < npair; e += 256) {                     // (a thread reads the counters it owns)
        const int r = e / k, t = e - r * k;
        if (i0 + r < N) a.ranks[(int64_t)(i0 + r) * a.ldr + t] = below[e];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define KNN_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

struct KnnSplit { int nsplit, tiles_per_split; };

// the database goes to one workgroup per 16 queries while those alone fill the device; fewer queries share it between up to 16
static KnnSplit knn_split(int64_t M, int64_t N) {
    const int blocks = (int)((M + KNN_ROWS - 1) / KNN_ROWS), tiles = (int)((N + KNN_COLS - 1) / KNN_COLS);
    int want = blocks >= 256 ? 1 : (512 + blocks - 1) / blocks;
    if (want > KNN_MAX_SPLIT) want = KNN_MAX_SPLIT;
    if (want > tiles) want = tiles;
    const int per = (tiles + want - 1) / want;
    return KnnSplit{(tiles + per - 1) / per, per};
}

static int knn_shape_check(int64_t M, int64_t N, int D, int k, const char* who) {
    KNN_REQUIRE(M >= 1 && M <= KNN_MAX_N && N >= 1 && N <= KNN_MAX_N, "%s: M=%lld, N=%lld (1 .. %d)", who, (long long)M, (long long)N, KNN_MAX_N);
    KNN_REQUIRE(D >= 1, "%s: D=%d (D >= 1)", who, D);
    KNN_REQUIRE(k >= 1 && k <= KNN_MAX_K && k <= N, "%s: k=%d (1 <= k <= %d, k <= N=%lld)", who, k, KNN_MAX_K, (long long)N);
    return 0;
}

int64_t knn_ws_bytes(int64_t M, int64_t N, int D, int k) {
    if (int rc = knn_shape_check(M, N, D, k, "dmvae_knn_ws_bytes")) return rc;
    const KnnSplit sp = knn_split(M, N);
    return sp.nsplit == 1 ? 0 : ((int64_t)sp.nsplit * M * k * (int64_t)sizeof(knn_key_t) + 255) & ~(int64_t)255;
}

int knn_launch(hipStream_t s, const float* Q, int64_t ldq, int M, const float* X, int64_t ldx, int N, int D, int k, int64_t self_first, void* ws,
               int64_t ws_bytes, int32_t* idx, float* d2, int64_t ldo) {
    const char* who = "dmvae_knn";
    if (int rc = knn_shape_check(M, N, D, k, who)) return rc;
    KNN_REQUIRE(Q && X && idx && d2, "%s: null Q / X / idx / d2", who);
    KNN_REQUIRE(ldq >= D && ldx >= D && ldo >= k, "%s: ldq=%lld, ldx=%lld, ldo=%lld (ldq >= D, ldx >= D, ldo >= k)", who, (long long)ldq, (long long)ldx,
                (long long)ldo);
    KNN_REQUIRE(k <= N - (self_first >= 0 ? 1 : 0), "%s: k=%d neighbours of N=%d rows with the row itself left out", who, k, N);
    const int64_t need = knn_ws_bytes(M, N, D, k);
    KNN_REQUIRE(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0),
                "%s: the workspace needs %lld bytes (dmvae_knn_ws_bytes), 8-byte aligned; got %lld at %p", who, (long long)need, (long long)ws_bytes, ws);
    const KnnSplit sp = knn_split(M, N);
    const int L = knn_list_len(k);
    static bool set = false;
    if (!set) {
        (void)hipFuncSetAttribute((const void*)knn_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        set = true;
    }
    ProfScope ps(s, "knn", (double)M * N * (3.0 * D + 2.0), 4.0 * N * ((double)D * ((M + KNN_ROWS - 1) / KNN_ROWS)) + 4.0 * M * (D + 2.0 * k));
    const KnnArgs a{Q, ldq, M, X, ldx, N, D, k, self_first, L, sp.tiles_per_split, sp.nsplit, sp.nsplit > 1 ? (knn_key_t*)ws : nullptr, idx, d2, ldo};
    DMVAE_LAUNCH(knn_pairs_kernel, dim3((M + KNN_ROWS - 1) / KNN_ROWS, sp.nsplit), dim3(256), knn_pairs_lds(L), s, a);
    if (sp.nsplit > 1)
        DMVAE_LAUNCH(knn_merge_kernel, dim3(M), dim3(64), (size_t)sp.nsplit * k * sizeof(knn_key_t), s, (const knn_key_t*)ws, M, k, sp.nsplit, idx, d2, ldo);
    return check_launch(who);
}

int knn_vote_launch(hipStream_t s, const int32_t* idx, int64_t ldi, int M, int k, const int32_t* classes, int N, int C, float* counts, int64_t ldc,
                    int32_t* err_flag) {
    const char* who = "dmvae_knn_vote";
    KNN_REQUIRE(idx && classes && counts && err_flag, "%s: null idx / classes / counts / err_flag", who);
    KNN_REQUIRE(M >= 1 && M <= KNN_MAX_N && N >= 1 && N <= KNN_MAX_N, "%s: M=%d, N=%d (1 .. %d)", who, M, N, KNN_MAX_N);
    KNN_REQUIRE(k >= 1 && k <= KNN_MAX_K && ldi >= k, "%s: k=%d, ldi=%lld (1 <= k <= %d, ldi >= k)", who, k, (long long)ldi, KNN_MAX_K);
    KNN_REQUIRE(C >= 1 && C <= KNN_MAX_C && ldc >= C, "%s: C=%d, ldc=%lld (1 <= C <= %d, ldc >= C)", who, C, (long long)ldc, KNN_MAX_C);
    ProfScope ps(s, "knn_vote", (double)M * k, 4.0 * M * (2.0 * k + C));
    DMVAE_LAUNCH(knn_vote_kernel, dim3(M), dim3(256), 0, s, idx, ldi, k, classes, N, C, counts, ldc, err_flag);
    return check_launch(who);
}

int knn_ranks_launch(hipStream_t s, const float* X, int64_t ldx, int N, int D, const int32_t* idx, int64_t ldi, int k, int32_t* ranks, int64_t ldr,
                     int32_t* err_flag) {
    const char* who = "dmvae_knn_ranks";
    KNN_REQUIRE(X && idx && ranks && err_flag, "%s: null X / idx / ranks / err_flag", who);
    KNN_REQUIRE(N >= 2 && N <= KNN_MAX_N && D >= 1 && ldx >= D, "%s: N=%d, D=%d, ldx=%lld (2 <= N <= %d, D >= 1, ldx >= D)", who, N, D, (long long)ldx,
                KNN_MAX_N);
    KNN_REQUIRE(k >= 1 && k <= KNN_MAX_K && k <= N - 1 && ldi >= k && ldr >= k, "%s: k=%d, ldi=%lld, ldr=%lld (1 <= k <= min(%d, N - 1), ldi >= k, ldr >= k)", who,
                k, (long long)ldi, (long long)ldr, KNN_MAX_K);
    static bool set = false;
    if (!set) {
        (void)hipFuncSetAttribute((const void*)knn_ranks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        set = true;
    }
    const size_t lds = (size_t)KNN_ROWS * k * (sizeof(knn_key_t) + sizeof(int)) + (size_t)KNN_ROWS * KNN_CKLD * sizeof(knn_key_t);
    ProfScope ps(s, "knn_ranks", (double)N * N * (3.0 * D + 2.0 * k), 4.0 * N * ((double)D * ((N + KNN_ROWS - 1) / KNN_ROWS)) + 8.0 * N * k);
    const KnnRankArgs a{X, ldx, N, D, idx, ldi, k, ranks, ldr, err_flag};
    DMVAE_LAUNCH(knn_ranks_kernel, dim3((N + KNN_ROWS - 1) / KNN_ROWS), dim3(256), lds, s, a);
    return check_launch(who);
}

}  // namespace dmvae
