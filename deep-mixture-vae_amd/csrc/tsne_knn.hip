// kNN-sparse t-SNE on the device: what sklearn.manifold.TSNE(method="barnes_hut") builds for P -- conditional probabilities over the
// k = min(N - 1, int(3 perplexity + 1)) nearest rows (dmvae_knn's lists), symmetrised over the union graph into CSR -- with the repulsive
// term kept EXACT over all pairs, so nothing but the truncation of P is approximated and no N x N array exists anywhere.
//   tsne_knn_cond_p_kernel   one wave per row: the row's k <= 256 shifted distances sit in four registers per lane; 64 bisection steps by
//                            the dense kernel's rule (s and the entropy's numerator in f64, beta / lo / hi in f32), then p_{j|i}
//   (the symmetrisation into CSR is a stable sort of int64 keys on the caller's side: dmvae_hip/tsne.py)
// and per iteration, five launches:
//   tsne_knn_attr_kernel     one wave per row over its CSR entries: sum_j P_ij q_ij (y_i - y_j), lanes in entry order, xor butterfly
//   tsne_knn_rep_kernel      all pairs: a thread owns row i and walks y_j from an LDS tile of <= 1024 columns (every lane reads the same
//                            address: a broadcast); f32 sums inside a tile, tiles joined in tile order (the q sum in f64).  The columns
//                            are dealt to gridDim.y = S splits in whole tiles; the partials lie [S][N]
//   tsne_knn_join_kernel     adds the S partials in split order and writes acc[i] = (ax, ay, rx, ry) and zrow[i] as the dense pass does
//   tsne_sum_kernel, tsne_update_kernel (tsne_grad_kernel)   of tsne.hip, unchanged
// The KL reuses the first four at the final Y, then tsne_knn_kl_kernel over the CSR entries (f64 terms) and tsne_sum_kernel.
// No float atomics, no host synchronisation, 64-bit entry offsets: two runs agree bit for bit.
#include <math.h>

#include "tsne.h"
#include "knn.h"

namespace dmvae {

struct TsneKnnWs {
    float2* attr;       // [N] sum_j P_ij q_ij (y_i - y_j)
    float2* prep;       // [S][N] the splits' sum_j q_ij^2 (y_i - y_j)
    double* pz;         // [S][N] the splits' sum_j q_ij
    float4* acc;        // [N] {attr_x, attr_y, rep_x, rep_y}
    double* zrow;       // [N]
    double* Z;          // [1]
    float* U;           // [N][2] the fit's velocity
    float* G;           // [N][2] the fit's gains
    double* klpart;     // [ceil(N / 4)]
};

__device__ __forceinline__ double tsne_knn_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int CP_SLOTS = KNN_MAX_K / 64;        // registers of one lane for its row's entries lane, lane + 64, ...

__global__ __launch_bounds__(256) void tsne_knn_cond_p_kernel(int N, int k, float perplexity, const float* __restrict__ d2, int64_t ldd, float* __restrict__ p,
                                                              int64_t ldp, float* __restrict__ beta_out) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                        // (no barrier in this kernel)
    const float* row = d2 + (int64_t)i * ldd;
    const float first = row[0];                                // the lists are ordered by (d2, j): the nearest comes first
    float d[CP_SLOTS];
#pragma unroll
    for (int t = 0; t < CP_SLOTS; ++t) {
        const int c = lane + 64 * t;
        d[t] = c < k ? row[c] - first : 0.f;
    }
    const double target = log((double)perplexity);
    float beta = 1.f, lo = 0.f, hi = 0.f;                      // lo = 0: (beta + lo) / 2 halves while no lower bound is known
    bool has_hi = false;
    double s = 1.0;
    for (int step = 0; step <= TSNE_SEARCH_STEPS; ++step) {    // the last trip only takes s at the final beta
        double ls = 0.0, ln = 0.0;
#pragma unroll
        for (int t = 0; t < CP_SLOTS; ++t) {
            if (lane + 64 * t < k) {
                const float e = expf(-beta * d[t]);
                ls += (double)e;
                ln += (double)(d[t] * e);
            }
        }
        s = tsne_knn_wave_sum(ls);                             // >= 1: the first neighbour contributes exp(0)
        if (step == TSNE_SEARCH_STEPS) break;
        const double H = log(s) + (double)beta * tsne_knn_wave_sum(ln) / s;
        if (H > target) {
            lo = beta;
            beta = has_hi ? (beta + hi) * 0.5f : beta * 2.f;
        } else {
            hi = beta;
            has_hi = true;
            beta = (beta + lo) * 0.5f;
        }
    }
    const float inv_s = (float)(1.0 / s);
    float* out = p + (int64_t)i * ldp;
#pragma unroll
    for (int t = 0; t < CP_SLOTS; ++t) {
        const int c = lane + 64 * t;
        if (c < k) out[c] = expf(-beta * d[t]) * inv_s;
    }
    if (lane == 0 && beta_out) beta_out[i] = beta;
}

// the entries [b, e) of row i, clamped into [0, nnz] so that a wrong indptr reads nothing outside the arrays
__device__ __forceinline__ void tsne_knn_row_range(const int64_t* __restrict__ indptr, int i, int64_t nnz, int64_t& b, int64_t& e) {
    b = indptr[i];
    e = indptr[i + 1];
    b = b < 0 ? 0 : b;
    e = e > nnz ? nnz : e;
}

__global__ __launch_bounds__(256) void tsne_knn_attr_kernel(int N, int64_t nnz, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ values, const float* __restrict__ Y, float2* __restrict__ attr) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                        // (no barrier in this kernel)
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    const float2 yi = Y2[i];
    int64_t b, e;
    tsne_knn_row_range(indptr, i, nnz, b, e);
    float ax = 0.f, ay = 0.f;
    for (int64_t t = b + lane; t < e; t += 64) {
        const int j = indices[t];
        if ((unsigned)j >= (unsigned)N) continue;              // (a column outside the rows is skipped, never read)
        const float2 yj = Y2[j];
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float pq = values[t] * __builtin_amdgcn_rcpf(1.f + dx * dx + dy * dy);
        ax += pq * dx;
        ay += pq * dy;
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (lane == 0) attr[i] = make_float2(ax, ay);
}

// the tiles [t0, t1) of split s among nt tiles: whole tiles, dealt as evenly as S allows (a split beyond the tiles is empty)
__host__ __device__ __forceinline__ void tsne_knn_split_tiles(int nt, int S, int s, int& t0, int& t1) {
    t0 = (int)((int64_t)nt * s / S);
    t1 = (int)((int64_t)nt * (s + 1) / S);
}

__global__ __launch_bounds__(256) void tsne_knn_rep_kernel(int N, const float* __restrict__ Y, float2* __restrict__ prep, double* __restrict__ pz) {
    __shared__ float2 tile[TSNE_KNN_TILE];
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid, s = blockIdx.y;
    const float2 yi = i < N ? Y2[i] : make_float2(0.f, 0.f);
    int t0, t1;
    tsne_knn_split_tiles((N + TSNE_KNN_TILE - 1) / TSNE_KNN_TILE, gridDim.y, s, t0, t1);
    float rx = 0.f, ry = 0.f;
    double z = 0.0;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * TSNE_KNN_TILE;
        const int cnt = N - j0 < TSNE_KNN_TILE ? N - j0 : TSNE_KNN_TILE;
        __syncthreads();                                       // the previous tile's reads are done
        for (int c = tid; c < cnt; c += 256) tile[c] = Y2[j0 + c];
        __syncthreads();
        const int self = i - j0;                               // the column of the tile that is row i itself, if any
        float tx = 0.f, ty = 0.f, tz = 0.f;
#pragma unroll 4
        for (int c = 0; c < cnt; ++c) {
            const float2 yj = tile[c];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float q = c == self ? 0.f : __builtin_amdgcn_rcpf(1.f + dx * dx + dy * dy);
            const float qq = q * q;
            tx += qq * dx;
            ty += qq * dy;
            tz += q;
        }
        rx += tx;
        ry += ty;
        z += (double)tz;
    }
    if (i < N) {
        prep[(int64_t)s * N + i] = make_float2(rx, ry);
        pz[(int64_t)s * N + i] = z;
    }
}

__global__ __launch_bounds__(256) void tsne_knn_join_kernel(int N, int S, const float2* __restrict__ attr, const float2* __restrict__ prep,
                                                            const double* __restrict__ pz, float4* __restrict__ acc, double* __restrict__ zrow) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float rx = 0.f, ry = 0.f;
    double z = 0.0;
    for (int s = 0; s < S; ++s) {
        const float2 r = prep[(int64_t)s * N + i];
        rx += r.x;
        ry += r.y;
        z += pz[(int64_t)s * N + i];
    }
    const float2 a = attr[i];
    acc[i] = make_float4(a.x, a.y, rx, ry);
    zrow[i] = z;
}

// sum over the CSR entries of P_ij log(P_ij Z (1 + |y_i - y_j|^2)), f64 terms: one partial per workgroup (four rows)
__global__ __launch_bounds__(256) void tsne_knn_kl_kernel(int N, int64_t nnz, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                          const float* __restrict__ values, const float* __restrict__ Y, const double* __restrict__ Zp,
                                                          double* __restrict__ part) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * 4 + w;
    double t = 0.0;
    if (i < N) {
        const float2* Y2 = reinterpret_cast<const float2*>(Y);
        const float2 yi = Y2[i];
        const double Z = Zp[0];
        int64_t b, e;
        tsne_knn_row_range(indptr, i, nnz, b, e);
        for (int64_t u = b + lane; u < e; u += 64) {
            const int j = indices[u];
            const float p = values[u];
            if ((unsigned)j < (unsigned)N && p > 0.f) {
                const float2 yj = Y2[j];
                const float dx = yi.x - yj.x, dy = yi.y - yj.y;
                t += (double)p * log((double)p * Z * (double)(1.f + dx * dx + dy * dy));
            }
        }
    }
    t = tsne_knn_wave_sum(t);
    if (lane == 0) red[w] = t;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int tsne_knn_k_of(int N, float perplexity) {
    const double k = floor(3.0 * (double)perplexity + 1.0);
    return k < (double)(N - 1) ? (int)k : N - 1;
}

int tsne_knn_check(const dmvae_tsne_knn_config* c, const char* who) {
    if (!c) {
        set_error("%s: null config", who);
        return DMVAE_EINVAL;
    }
    if (c->N < 4 || c->N > KNN_MAX_N || !(c->perplexity > 1.f) || !(c->perplexity < (float)(c->N - 1)) || c->n_iter < 0 || c->exaggeration_iters < 0 ||
        c->flags != 0 || !(c->early_exaggeration > 0.f) || !(c->learning_rate > 0.f) || c->col_splits < 0 || c->col_splits > TSNE_KNN_MAX_SPLITS ||
        c->nnz < 0) {
        set_error("%s: needs 4 <= N <= %d, 1 < perplexity < N - 1, n_iter >= 0, exaggeration_iters >= 0, early_exaggeration > 0, learning_rate > 0, "
                  "0 <= col_splits <= %d, nnz >= 0 and flags 0; got N=%d perplexity=%g n_iter=%d exaggeration_iters=%d early_exaggeration=%g "
                  "learning_rate=%g col_splits=%d nnz=%lld flags=%d", who, KNN_MAX_N, TSNE_KNN_MAX_SPLITS, c->N, (double)c->perplexity, c->n_iter,
                  c->exaggeration_iters, (double)c->early_exaggeration, (double)c->learning_rate, c->col_splits, (long long)c->nnz, c->flags);
        return DMVAE_EINVAL;
    }
    const int k = tsne_knn_k_of(c->N, c->perplexity);
    if (k > KNN_MAX_K) {
        set_error("%s: perplexity=%g needs k = min(N - 1, int(3 perplexity + 1)) = %d neighbours, above dmvae_knn's cap of %d (perplexity above 85)", who,
                  (double)c->perplexity, k, KNN_MAX_K);
        return DMVAE_EINVAL;
    }
    if (c->k != k) {
        set_error("%s: k=%d, but min(N - 1, int(3 perplexity + 1)) = %d for N=%d perplexity=%g", who, c->k, k, c->N, (double)c->perplexity);
        return DMVAE_EINVAL;
    }
    return 0;
}

// host arithmetic on N alone: enough workgroups of 256 rows for eight per compute unit of a 256-unit part, in whole tiles
int tsne_knn_splits(const dmvae_tsne_knn_config* c) {
    if (c->col_splits > 0) return c->col_splits;
    const int blocks = (c->N + 255) / 256, nt = (c->N + TSNE_KNN_TILE - 1) / TSNE_KNN_TILE;
    int S = (2048 + blocks - 1) / blocks;
    S = S < nt ? S : nt;
    S = S < TSNE_KNN_MAX_SPLITS ? S : TSNE_KNN_MAX_SPLITS;
    return S < 1 ? 1 : S;
}

static int64_t tsne_knn_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

static int64_t tsne_knn_carve(const dmvae_tsne_knn_config* c, char* base, TsneKnnWs* w) {
    const int64_t N = c->N, S = tsne_knn_splits(c);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += tsne_knn_up256(bytes); return p; };
    TsneKnnWs t;
    t.attr = (float2*)take(N * 8);
    t.prep = (float2*)take(S * N * 8);
    t.pz = (double*)take(S * N * 8);
    t.acc = (float4*)take(N * 16);
    t.zrow = (double*)take(N * 8);
    t.Z = (double*)take(8);
    t.U = (float*)take(N * 8);
    t.G = (float*)take(N * 8);
    t.klpart = (double*)take((N + 3) / 4 * 8);
    if (w) *w = t;
    return off;
}

int64_t tsne_knn_ws_bytes(const dmvae_tsne_knn_config* c) { return tsne_knn_carve(c, nullptr, nullptr); }

static int tsne_knn_ws_check(const dmvae_tsne_knn_config* c, const void* ws, int64_t ws_bytes, const char* who) {
    if (!ws || ws_bytes < tsne_knn_ws_bytes(c) || ((uintptr_t)ws & 15)) {
        set_error("%s: the workspace needs %lld bytes (dmvae_tsne_knn_ws_bytes), 16-byte aligned; got %lld at %p", who, (long long)tsne_knn_ws_bytes(c),
                  (long long)ws_bytes, ws);
        return DMVAE_EINVAL;
    }
    return 0;
}

static int tsne_knn_csr_check(const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, const char* who) {
    if (!indptr || ((uintptr_t)indptr & 7) || (c->nnz > 0 && (!indices || !values))) {
        set_error("%s: indptr (8-byte aligned), indices and values must be given", who);
        return DMVAE_EINVAL;
    }
    return 0;
}

static int tsne_knn_rows_grid(int N) { return (N + 3) / 4; }

// the rows' attractive / repulsive sums and Z at Y: four launches
static void tsne_knn_pairs_enqueue(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values,
                                   const TsneKnnWs& w, const float* Y) {
    const int N = c->N, S = tsne_knn_splits(c);
    DMVAE_LAUNCH(tsne_knn_attr_kernel, dim3(tsne_knn_rows_grid(N)), dim3(256), 0, s, N, c->nnz, indptr, indices, values, Y, w.attr);
    DMVAE_LAUNCH(tsne_knn_rep_kernel, dim3((N + 255) / 256, S), dim3(256), 0, s, N, Y, w.prep, w.pz);
    DMVAE_LAUNCH(tsne_knn_join_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, S, w.attr, w.prep, w.pz, w.acc, w.zrow);
    DMVAE_LAUNCH(tsne_sum_kernel, dim3(1), dim3(256), 0, s, w.zrow, N, w.Z);
}

static void tsne_knn_step_enqueue(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values,
                                  const TsneKnnWs& w, float* Y, float* U, float* G, float e, float m) {
    const int N = c->N;
    ProfScope ps(s, "tsne_knn_step", (double)N * N * 12.0 + (double)c->nnz * 10.0, (double)c->nnz * 16.0);
    tsne_knn_pairs_enqueue(s, c, indptr, indices, values, w, Y);
    DMVAE_LAUNCH(tsne_update_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, w.acc, w.Z, e, m, c->learning_rate, Y, U, G);
}

int tsne_knn_cond_p_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const float* d2, int64_t ldd, float* p, int64_t ldp, float* beta) {
    const char* who = "dmvae_tsne_knn_cond_p";
    if (int rc = tsne_knn_check(c, who)) return rc;
    if (!d2 || !p || ldd < c->k || ldp < c->k) {
        set_error("%s: d2 and p must be given with ldd >= k and ldp >= k", who);
        return DMVAE_EINVAL;
    }
    ProfScope ps(s, "tsne_knn_cond_p", (double)c->N * c->k * 12.0 * (TSNE_SEARCH_STEPS + 2), (double)c->N * c->k * 8.0);
    DMVAE_LAUNCH(tsne_knn_cond_p_kernel, dim3(tsne_knn_rows_grid(c->N)), dim3(256), 0, s, c->N, c->k, c->perplexity, d2, ldd, p, ldp, beta);
    return check_launch(who);
}

int tsne_knn_gradient_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, void* ws,
                             int64_t ws_bytes, const float* Y, float exaggeration, float* grad) {
    const char* who = "dmvae_tsne_knn_gradient";
    if (int rc = tsne_knn_check(c, who)) return rc;
    if (int rc = tsne_knn_csr_check(c, indptr, indices, values, who)) return rc;
    if (!Y || !grad || ((uintptr_t)Y & 7) || ((uintptr_t)grad & 7)) {
        set_error("%s: Y and grad must be given, 8-byte aligned", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_knn_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneKnnWs w;
    tsne_knn_carve(c, (char*)ws, &w);
    tsne_knn_pairs_enqueue(s, c, indptr, indices, values, w, Y);
    DMVAE_LAUNCH(tsne_grad_kernel, dim3((c->N + 255) / 256), dim3(256), 0, s, c->N, w.acc, w.Z, exaggeration, grad);
    return check_launch(who);
}

int tsne_knn_step_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, void* ws,
                         int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration, float momentum) {
    const char* who = "dmvae_tsne_knn_step";
    if (int rc = tsne_knn_check(c, who)) return rc;
    if (int rc = tsne_knn_csr_check(c, indptr, indices, values, who)) return rc;
    if (!Y || !U || !G || (((uintptr_t)Y | (uintptr_t)U | (uintptr_t)G) & 7)) {
        set_error("%s: Y, U and G must be given, 8-byte aligned", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_knn_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneKnnWs w;
    tsne_knn_carve(c, (char*)ws, &w);
    tsne_knn_step_enqueue(s, c, indptr, indices, values, w, Y, U, G, exaggeration, momentum);
    return check_launch(who);
}

int tsne_knn_fit_launch(hipStream_t s, const dmvae_tsne_knn_config* c, const int64_t* indptr, const int32_t* indices, const float* values, const float* Y0,
                        void* ws, int64_t ws_bytes, float* Y, double* kl) {
    const char* who = "dmvae_tsne_knn_fit";
    if (int rc = tsne_knn_check(c, who)) return rc;
    if (int rc = tsne_knn_csr_check(c, indptr, indices, values, who)) return rc;
    if (!Y || !kl || ((uintptr_t)Y & 7) || ((uintptr_t)kl & 7)) {
        set_error("%s: Y and kl must be given, 8-byte aligned", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_knn_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneKnnWs w;
    tsne_knn_carve(c, (char*)ws, &w);
    const int N = c->N;
    DMVAE_LAUNCH(tsne_init_kernel, dim3((2 * N + 255) / 256), dim3(256), 0, s, 2 * N, Y0, c->seed, Y, w.U, w.G);
    for (int it = 0; it < c->n_iter; ++it) {
        const bool early = it < c->exaggeration_iters;
        tsne_knn_step_enqueue(s, c, indptr, indices, values, w, Y, w.U, w.G, early ? c->early_exaggeration : 1.f, early ? 0.5f : 0.8f);
    }
    tsne_knn_pairs_enqueue(s, c, indptr, indices, values, w, Y);
    DMVAE_LAUNCH(tsne_knn_kl_kernel, dim3(tsne_knn_rows_grid(N)), dim3(256), 0, s, N, c->nnz, indptr, indices, values, Y, w.Z, w.klpart);
    DMVAE_LAUNCH(tsne_sum_kernel, dim3(1), dim3(256), 0, s, w.klpart, tsne_knn_rows_grid(N), kl);
    return check_launch(who);
}

}  // namespace dmvae
