// Diagonal-covariance Gaussian mixture fit: the GMM initialisation of the prior tables (code/base_models.py:367-390, 614-646 call
// sklearn.mixture.GaussianMixture(covariance_type="diag") on the encoder means of the whole data set), n_init restarts side by side.
//   E: lp_nk = log w_k - 1/2 [D log 2pi + sum_d log var_kd + sum_d (x_nd - mu_kd)^2 / var_kd],  ll_n = logsumexp_k lp_nk,  resp = exp(lp - ll)
//   M: nk = sum_n resp + 10 eps,  w = nk / sum nk,  mu = sum resp x / nk,  var = sum resp x^2 / nk - mu^2 + reg_covar
// Two kernels per iteration, the restart in the grid's second dimension:
//   gmm_rows_kernel      a workgroup walks its rows in tiles of 32.  Row stage: 16 lanes per row (lane owns k = lane + 16 j), the restart's tables
//                        and the tile in LDS; resp is soft (EM), one-hot of given labels (the initial M-step), one-hot of the nearest centre
//                        (Lloyd; first index on ties; writes the labels) or all on component 0 (the column variances Lloyd's stopping rule
//                        needs).  Statistics: thread t owns the pairs (k, d) = t + 256 j and walks the tile's rows in order -- no cross-lane
//                        reduction, no atomics -- accumulating about the CURRENT mean:
//                            S0_k = sum resp,  S1_kd = sum resp (x - mu_kd),  S2_kd = sum resp (x - mu_kd)^2,  sum ll_n
//                        so that f32 sums do not cancel the way E[x^2] - mu^2 does.  Per-workgroup partials [R][nblk][K + 2 K D].
//   gmm_finalize_kernel  one workgroup per restart adds the partials in block order in f64 and updates the tables.  With a = S0 / nk,
//                        m1 = S1 / nk, m2 = S2 / nk the shifted sums give exactly
//                            mu' = a mu + m1,   var' = m2 - m1^2 + 2 mu m1 (1 - a) + a (1 - a) mu^2 + reg_covar
//                        (a = 1 - 10 eps / nk: an empty component gets mean 0 and variance reg_covar as in sklearn).  It also writes what the
//                        next row stage reads (1 / var and c_k = log w_k - 1/2 [D log 2pi + sum_d log var_kd]), the lower bound, the iteration
//                        count and the done flag; a restart that is done is frozen: its workgroups of later launches return on the flag.
// The loop is issued whole (max_iter rounds), without a host synchronisation; gmm_select_kernel copies the restart with the largest bound.
#include <math.h>

#include "gmm_fit.h"
#include "latent_body.h"

namespace dmvae {

enum { GMM_SOFT = 0, GMM_LABELS = 1, GMM_ARGMIN = 2, GMM_CONST0 = 3 };
enum { GMM_FIN_EM = 0, GMM_FIN_INIT = 1, GMM_FIN_LLOYD = 2, GMM_FIN_XVAR = 3 };

struct GmmWs {
    float *w, *mu, *var, *iv, *ck;      // [R][K], [R][K][D] x 3, [R][K]
    float* part;                        // [R][nblk][K + 2 K D]
    double* llpart;                     // [R][nblk]
    int* nchg;                          // [R][nblk] labels that changed (Lloyd)
    double* lb;                         // [R]
    double* xvar;                       // [1] mean_d Var(X_d)
    int *n_iter, *done, *conv, *km_iter, *km_done;      // [R]
    int* labels;                        // [R][N]
};

struct GmmArgs {
    int N, D, K, R, nblk, tiles_per_blk, mode;
    int64_t ldx;
    const float* X;
    const int* labels_in;               // GMM_LABELS: [R][N]
    const int* done;                    // restarts to skip (null: none)
    const float* weights_init;          // GMM_FIN_INIT: [K] or null
    double tol, reg;
    GmmWs ws;
};

static size_t gmm_rows_lds(int D, int K) {
    return 256 + sizeof(float) * ((size_t)2 * K * (D + 1) + K + (size_t)GMM_TILE_ROWS * (D + 1) + (size_t)GMM_TILE_ROWS * (K + 1));
}

__global__ __launch_bounds__(256) void gmm_fill_kernel(float* mu, const float* X, int D, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mu[i] = X[i % D];        // every component's shift point: row 0 of X
}

template <int MODE>
__global__ __launch_bounds__(256) void gmm_rows_kernel(GmmArgs a) {
    const int r = blockIdx.y;
    if (a.done && a.done[r]) return;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int TR = GMM_TILE_ROWS, PPT = GMM_PAIRS_PER_THREAD;
    const int K = a.K, D = a.D, DP = D + 1, KP = K + 1, KD = K * D, N = a.N;
    double* red = reinterpret_cast<double*>(lds);      // [32]
    float* tmu = lds + 64;            // [K][DP] means / centres
    float* tiv = tmu + K * DP;        // [K][DP] 1 / var
    float* tck = tiv + K * DP;        // [K] log w_k - 1/2 [D log 2pi + sum_d log var_kd]
    float* xt = tck + K;              // [TR][DP] the tile's rows
    float* rs = xt + TR * DP;         // [TR][KP] their resp

    const int tid = threadIdx.x, lr = tid & 15, rsub = tid >> 4;
    const float* gmu = a.ws.mu + (int64_t)r * KD;
    for (int idx = tid; idx < KD; idx += 256) {
        const int k = idx / D, d = idx - k * D;
        tmu[k * DP + d] = gmu[idx];
        tiv[k * DP + d] = MODE == GMM_SOFT ? a.ws.iv[(int64_t)r * KD + idx] : 1.f;
    }
    for (int k = tid; k < K; k += 256) tck[k] = MODE == GMM_SOFT ? a.ws.ck[(int64_t)r * K + k] : 0.f;
    __syncthreads();

    int pk[PPT], pd[PPT];
    float pm[PPT], s1[PPT], s2[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int idx = tid + 256 * j;
        const int k = idx < KD ? idx / D : 0, d = idx < KD ? idx - k * D : 0;
        pk[j] = k; pd[j] = d; pm[j] = tmu[k * DP + d];
        s1[j] = 0.f; s2[j] = 0.f;
    }
    float s0 = 0.f;
    double llacc = 0.0;
    int chg = 0;

    const int tile0 = blockIdx.x * a.tiles_per_blk;
    for (int t = 0; t < a.tiles_per_blk; ++t) {
        const int row0 = (tile0 + t) * TR;
        if (row0 >= N) break;
        __syncthreads();              // the walk over the previous tile is over
        for (int idx = tid; idx < TR * D; idx += 256) {
            const int rr = idx / D, d = idx - rr * D;
            const int n = row0 + rr;
            xt[rr * DP + d] = n < N ? a.X[(int64_t)n * a.ldx + d] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < TR / 16; ++pass) {
            const int rr = rsub + 16 * pass;
            const int n = row0 + rr;
            const bool valid = n < N;
            const float* xr = xt + rr * DP;
            if (MODE == GMM_SOFT) {
                float mx = -INFINITY;
                for (int k = lr; k < K; k += 16) {
                    float q = 0.f;
                    for (int d = 0; d < D; ++d) {
                        const float dx = xr[d] - tmu[k * DP + d];
                        q += dx * dx * tiv[k * DP + d];
                    }
                    const float lp = tck[k] - 0.5f * q;
                    rs[rr * KP + k] = lp;
                    mx = fmaxf(mx, lp);
                }
                mx = row_max16(mx);
                float se = 0.f;
                for (int k = lr; k < K; k += 16) {
                    const float ex = __expf(rs[rr * KP + k] - mx);
                    rs[rr * KP + k] = ex;
                    se += ex;
                }
                se = row_sum16(se);
                const float inv = 1.f / se;
                for (int k = lr; k < K; k += 16) rs[rr * KP + k] = valid ? rs[rr * KP + k] * inv : 0.f;
                if (lr == 0 && valid) llacc += (double)(mx + __logf(se));
            } else if (MODE == GMM_ARGMIN) {
                float best = INFINITY;
                int bk = K;
                for (int k = lr; k < K; k += 16) {
                    float q = 0.f;
                    for (int d = 0; d < D; ++d) {
                        const float dx = xr[d] - tmu[k * DP + d];
                        q += dx * dx;
                    }
                    if (q < best) { best = q; bk = k; }
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    const float ob = __shfl_xor(best, o, 16);
                    const int ok = __shfl_xor(bk, o, 16);
                    if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; }
                }
                for (int k = lr; k < K; k += 16) rs[rr * KP + k] = (valid && k == bk) ? 1.f : 0.f;
                if (lr == 0 && valid) {
                    int* lab = a.ws.labels + (int64_t)r * N + n;
                    chg += *lab != bk;
                    *lab = bk;
                }
            } else {
                int lab = -1;
                if (valid) lab = MODE == GMM_LABELS ? a.labels_in[(int64_t)r * N + n] : 0;
                for (int k = lr; k < K; k += 16) rs[rr * KP + k] = k == lab ? 1.f : 0.f;
            }
        }
        __syncthreads();
        for (int rr = 0; rr < TR; ++rr) {
#pragma unroll
            for (int j = 0; j < PPT; ++j) {
                if (256 * j < KD) {
                    const float dx = xt[rr * DP + pd[j]] - pm[j];
                    const float wx = rs[rr * KP + pk[j]] * dx;
                    s1[j] += wx;
                    s2[j] += wx * dx;
                }
            }
            if (tid < K) s0 += rs[rr * KP + tid];
        }
    }

    const int P = K + 2 * KD;
    float* part = a.ws.part + ((int64_t)r * a.nblk + blockIdx.x) * P;
    if (tid < K) part[tid] = s0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int idx = tid + 256 * j;
        if (idx < KD) { part[K + idx] = s1[j]; part[K + KD + idx] = s2[j]; }
    }
    __syncthreads();
    if (lr == 0) { red[rsub] = llacc; red[16 + rsub] = (double)chg; }
    __syncthreads();
    if (tid == 0) {
        double l = 0.0, c = 0.0;
        for (int i = 0; i < 16; ++i) { l += red[i]; c += red[16 + i]; }
        a.ws.llpart[(int64_t)r * a.nblk + blockIdx.x] = l;
        a.ws.nchg[(int64_t)r * a.nblk + blockIdx.x] = (int)c;
    }
}

template <int FIN>
__global__ __launch_bounds__(256) void gmm_finalize_kernel(GmmArgs a) {
    const int r = blockIdx.x;
    if (a.done && a.done[r]) return;
    extern __shared__ __attribute__((aligned(16))) double fl[];
    const int K = a.K, D = a.D, KD = K * D, P = K + 2 * KD, tid = threadIdx.x;
    double* S0 = fl;              // [K]
    double* acc = S0 + K;         // [K][D]
    double* misc = acc + KD;      // [2]
    const double eps10 = 10.0 * 2.220446049250313e-16;
    const float* part = a.ws.part + (int64_t)r * a.nblk * P;
    for (int k = tid; k < K; k += 256) {
        double s = 0.0;
        for (int b = 0; b < a.nblk; ++b) s += (double)part[(int64_t)b * P + k];
        S0[k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int k = 0; k < K; ++k) tot += S0[k] + eps10;
        misc[0] = tot;
    }
    float* gmu = a.ws.mu + (int64_t)r * KD;
    for (int idx = tid; idx < KD; idx += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int b = 0; b < a.nblk; ++b) {
            t1 += (double)part[(int64_t)b * P + K + idx];
            t2 += (double)part[(int64_t)b * P + K + KD + idx];
        }
        const int k = idx / D;
        const double mu = (double)gmu[idx];
        if (FIN == GMM_FIN_LLOYD) {
            const float m32 = (float)(S0[k] > 0.0 ? mu + t1 / S0[k] : mu);       // an empty cluster keeps its centre
            const double dd = (double)m32 - mu;
            acc[idx] = dd * dd;
            gmu[idx] = m32;
        } else if (FIN == GMM_FIN_XVAR) {
            const double m1 = t1 / a.N;
            acc[idx] = t2 / a.N - m1 * m1;
        } else {
            const double nk = S0[k] + eps10, f = S0[k] / nk, m1 = t1 / nk, m2 = t2 / nk;
            const double v = m2 - m1 * m1 + 2.0 * mu * m1 * (1.0 - f) + f * (1.0 - f) * mu * mu + a.reg;
            const float v32 = (float)v;
            gmu[idx] = (float)(f * mu + m1);
            a.ws.var[(int64_t)r * KD + idx] = v32;
            a.ws.iv[(int64_t)r * KD + idx] = (float)(1.0 / (double)v32);
            acc[idx] = log((double)v32);
        }
    }
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s += acc[k * D + d];
        if (FIN == GMM_FIN_EM || FIN == GMM_FIN_INIT) {
            const float w32 = (FIN == GMM_FIN_INIT && a.weights_init) ? a.weights_init[k] : (float)((S0[k] + eps10) / misc[0]);
            a.ws.w[(int64_t)r * K + k] = w32;
            a.ws.ck[(int64_t)r * K + k] = (float)(log((double)w32) - 0.5 * (D * 1.8378770664093453 + s));
        }
        S0[k] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    if (FIN == GMM_FIN_EM) {
        double ll = 0.0;
        for (int b = 0; b < a.nblk; ++b) ll += a.ws.llpart[(int64_t)r * a.nblk + b];
        const double lb = ll / a.N, prev = a.ws.lb[r];
        a.ws.lb[r] = lb;
        a.ws.n_iter[r] += 1;
        if (fabs(lb - prev) < a.tol) { a.ws.conv[r] = 1; a.ws.done[r] = 1; }
    } else if (FIN == GMM_FIN_INIT) {
        a.ws.lb[r] = -INFINITY;
        a.ws.n_iter[r] = 0; a.ws.conv[r] = 0; a.ws.done[r] = 0;
    } else if (FIN == GMM_FIN_LLOYD) {
        double shift = 0.0;
        for (int k = 0; k < K; ++k) shift += S0[k];
        long long chg = 0;
        for (int b = 0; b < a.nblk; ++b) chg += a.ws.nchg[(int64_t)r * a.nblk + b];
        a.ws.km_iter[r] += 1;
        if (chg == 0 || shift <= 1e-4 * a.ws.xvar[0]) a.ws.km_done[r] = 1;
    } else {
        a.ws.xvar[0] = S0[0] / D;
    }
}

__global__ __launch_bounds__(256) void gmm_select_kernel(GmmArgs a, dmvae_gmm_result o) {
    __shared__ int sbest;
    const int K = a.K, KD = a.K * a.D, R = a.R, tid = threadIdx.x;
    if (tid == 0) {
        int best = 0;
        for (int r = 1; r < R; ++r)
            if (a.ws.lb[r] > a.ws.lb[best]) best = r;      // strict: the first restart wins a tie
        sbest = best;
        *o.lower_bound = a.ws.lb[best];
        *o.n_iter = a.ws.n_iter[best];
        *o.converged = a.ws.conv[best];
        *o.best_restart = best;
    }
    __syncthreads();
    const int best = sbest;
    for (int i = tid; i < K; i += 256) o.weights[i] = a.ws.w[(int64_t)best * K + i];
    for (int i = tid; i < KD; i += 256) {
        o.means[i] = a.ws.mu[(int64_t)best * KD + i];
        o.covariances[i] = a.ws.var[(int64_t)best * KD + i];
    }
    for (int i = tid; i < R; i += 256) {
        if (o.lower_bounds) o.lower_bounds[i] = a.ws.lb[i];
        if (o.n_iters) o.n_iters[i] = a.ws.n_iter[i];
        if (o.convergeds) o.convergeds[i] = a.ws.conv[i];
    }
    for (int i = tid; i < R * K; i += 256)
        if (o.all_weights) o.all_weights[i] = a.ws.w[i];
    for (int i = tid; i < R * KD; i += 256) {
        if (o.all_means) o.all_means[i] = a.ws.mu[i];
        if (o.all_covariances) o.all_covariances[i] = a.ws.var[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int gmm_blocks(int N, int* tiles_per_blk) {
    const int ntiles = (N + GMM_TILE_ROWS - 1) / GMM_TILE_ROWS;
    const int tpb = (ntiles + GMM_MAX_BLOCKS - 1) / GMM_MAX_BLOCKS;
    *tiles_per_blk = tpb;
    return (ntiles + tpb - 1) / tpb;
}

int gmm_check(const dmvae_gmm_config* c, const char* who) {
    if (!c || c->N < 1 || c->D < 1 || c->K < 1 || c->n_init < 1 || c->max_iter < 1 || c->kmeans_iter < 0 || c->flags != 0 || !(c->tol >= 0.f) ||
        !(c->reg_covar >= 0.f)) {
        set_error("%s: N, D, K, n_init, max_iter must be >= 1, kmeans_iter, tol, reg_covar >= 0 and flags 0", who);
        return DMVAE_EINVAL;
    }
    if ((int64_t)c->n_init * c->N > INT32_MAX || (int64_t)c->n_init * c->K * c->D > INT32_MAX || c->n_init > 65535) {
        set_error("%s: n_init * N and n_init * K * D must fit 31 bits, n_init <= 65535", who);
        return DMVAE_EINVAL;
    }
    const size_t lb = gmm_rows_lds(c->D, c->K);
    if ((int64_t)c->K * c->D > 256 * GMM_PAIRS_PER_THREAD || c->K > 256 || lb > 65536) {
        set_error("%s: K=%d D=%d needs K * D <= %d, K <= 256 and %zu <= 65536 B of LDS (tables and a %d-row tile live in LDS)", who, c->K, c->D,
                  256 * GMM_PAIRS_PER_THREAD, lb, GMM_TILE_ROWS);
        return DMVAE_EUNSUPPORTED;
    }
    return 0;
}

static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// the workspace's arrays, in order; base == nullptr: only the total
static int64_t gmm_carve(const dmvae_gmm_config* c, char* base, GmmWs* w) {
    int tpb;
    const int64_t R = c->n_init, K = c->K, KD = (int64_t)c->K * c->D, nblk = gmm_blocks(c->N, &tpb), P = K + 2 * KD;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += up256(bytes); return p; };
    GmmWs t;
    t.w = (float*)take(R * K * 4); t.mu = (float*)take(R * KD * 4); t.var = (float*)take(R * KD * 4); t.iv = (float*)take(R * KD * 4);
    t.ck = (float*)take(R * K * 4);
    t.part = (float*)take(R * nblk * P * 4);
    t.llpart = (double*)take(R * nblk * 8);
    t.nchg = (int*)take(R * nblk * 4);
    t.lb = (double*)take(R * 8);
    t.xvar = (double*)take(8);
    t.n_iter = (int*)take(R * 4); t.done = (int*)take(R * 4); t.conv = (int*)take(R * 4); t.km_iter = (int*)take(R * 4); t.km_done = (int*)take(R * 4);
    t.labels = (int*)take(R * c->N * 4);
    if (w) *w = t;
    return off;
}

int64_t gmm_ws_bytes(const dmvae_gmm_config* c) { return gmm_carve(c, nullptr, nullptr); }

static void gmm_rows(hipStream_t s, int mode, const GmmArgs& a) {
    const dim3 grid(a.nblk, a.R), block(256);
    const size_t lds = gmm_rows_lds(a.D, a.K);
    if (mode == GMM_SOFT) DMVAE_LAUNCH(gmm_rows_kernel<GMM_SOFT>, grid, block, lds, s, a);
    else if (mode == GMM_LABELS) DMVAE_LAUNCH(gmm_rows_kernel<GMM_LABELS>, grid, block, lds, s, a);
    else if (mode == GMM_ARGMIN) DMVAE_LAUNCH(gmm_rows_kernel<GMM_ARGMIN>, grid, block, lds, s, a);
    else DMVAE_LAUNCH(gmm_rows_kernel<GMM_CONST0>, grid, block, lds, s, a);
}

static void gmm_finalize(hipStream_t s, int fin, const GmmArgs& a) {
    const dim3 grid(a.R), block(256);
    const size_t lds = sizeof(double) * ((size_t)a.K + (size_t)a.K * a.D + 2);
    if (fin == GMM_FIN_EM) DMVAE_LAUNCH(gmm_finalize_kernel<GMM_FIN_EM>, grid, block, lds, s, a);
    else if (fin == GMM_FIN_INIT) DMVAE_LAUNCH(gmm_finalize_kernel<GMM_FIN_INIT>, grid, block, lds, s, a);
    else if (fin == GMM_FIN_LLOYD) DMVAE_LAUNCH(gmm_finalize_kernel<GMM_FIN_LLOYD>, grid, block, lds, s, a);
    else DMVAE_LAUNCH(gmm_finalize_kernel<GMM_FIN_XVAR>, grid, block, lds, s, a);
}

#define GMM_HIP(call, what)                                                  \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            set_error("%s: %s: %s", who, what, hipGetErrorString(e_));       \
            return (int)e_;                                                  \
        }                                                                    \
    } while (0)

int gmm_fit_launch(hipStream_t s, const dmvae_gmm_config* c, const float* X, int64_t ldx, const int32_t* labels, const float* centers,
                   const float* weights_init, void* ws, int64_t ws_bytes, const dmvae_gmm_result* out, bool kmeans_only) {
    const char* who = kmeans_only ? "dmvae_gmm_kmeans" : "dmvae_gmm_fit";
    if (int rc = gmm_check(c, who)) return rc;
    if (!X || !ws || !out || ldx < c->D || ((labels != nullptr) == (centers != nullptr))) {
        set_error("%s: X, ws, out must be given, ldx >= D, and exactly one of labels / centers", who);
        return DMVAE_EINVAL;
    }
    if (kmeans_only ? !(out->centers && out->labels)
                    : !(out->weights && out->means && out->covariances && out->lower_bound && out->n_iter && out->converged && out->best_restart)) {
        set_error("%s: a required pointer of the result is null", who);
        return DMVAE_EINVAL;
    }
    if (ws_bytes < gmm_ws_bytes(c) || ((uintptr_t)ws & 7)) {
        set_error("%s: the workspace needs %lld bytes (dmvae_gmm_ws_bytes), 8-byte aligned; got %lld", who, (long long)gmm_ws_bytes(c), (long long)ws_bytes);
        return DMVAE_EINVAL;
    }
    const int N = c->N, D = c->D, K = c->K, R = c->n_init;
    const int64_t KD = (int64_t)K * D;
    GmmArgs a{};
    a.N = N; a.D = D; a.K = K; a.R = R;
    a.nblk = gmm_blocks(N, &a.tiles_per_blk);
    a.ldx = ldx; a.X = X;
    a.weights_init = weights_init;
    a.tol = (double)c->tol; a.reg = (double)c->reg_covar;
    gmm_carve(c, (char*)ws, &a.ws);
    const double rows = (double)R * N;
    ProfScope ps(s, kmeans_only ? "gmm_kmeans" : "gmm_fit", rows * KD * 9.0 * c->max_iter, rows * D * 4.0 * c->max_iter);

    if (centers) {
        // mean_d Var(X_d) for Lloyd's stopping rule: the statistics of one component that owns every row, about row 0
        GmmArgs v = a;
        v.K = 1; v.R = 1;
        DMVAE_LAUNCH(gmm_fill_kernel, dim3((D + 255) / 256), dim3(256), 0, s, a.ws.mu, X, D, (int64_t)D);
        gmm_rows(s, GMM_CONST0, v);
        gmm_finalize(s, GMM_FIN_XVAR, v);
        GMM_HIP(hipMemcpyAsync(a.ws.mu, centers, R * KD * 4, hipMemcpyDeviceToDevice, s), "copying the centres");
        GMM_HIP(hipMemsetAsync(a.ws.labels, 0xFF, (size_t)R * N * 4, s), "labels = -1");
        GMM_HIP(hipMemsetAsync(a.ws.km_iter, 0, up256(R * 4) + (size_t)R * 4, s), "clearing the Lloyd state");      // km_iter and km_done, adjacent
        GmmArgs l = a;
        l.done = a.ws.km_done;
        for (int it = 0; it < c->kmeans_iter; ++it) {
            gmm_rows(s, GMM_ARGMIN, l);
            gmm_finalize(s, GMM_FIN_LLOYD, l);
        }
        gmm_rows(s, GMM_ARGMIN, a);       // the labels of the final centres (every restart)
        if (out->centers) GMM_HIP(hipMemcpyAsync(out->centers, a.ws.mu, R * KD * 4, hipMemcpyDeviceToDevice, s), "copying the centres out");
        if (out->labels) GMM_HIP(hipMemcpyAsync(out->labels, a.ws.labels, (size_t)R * N * 4, hipMemcpyDeviceToDevice, s), "copying the labels out");
        if (out->kmeans_iters) GMM_HIP(hipMemcpyAsync(out->kmeans_iters, a.ws.km_iter, R * 4, hipMemcpyDeviceToDevice, s), "copying the iteration counts out");
        if (kmeans_only) return check_launch(who);
        a.labels_in = a.ws.labels;
    } else {
        a.labels_in = labels;
    }
    DMVAE_LAUNCH(gmm_fill_kernel, dim3((unsigned)((R * KD + 255) / 256)), dim3(256), 0, s, a.ws.mu, X, D, R * KD);
    gmm_rows(s, GMM_LABELS, a);
    gmm_finalize(s, GMM_FIN_INIT, a);
    a.done = a.ws.done;
    for (int it = 0; it < c->max_iter; ++it) {
        gmm_rows(s, GMM_SOFT, a);
        gmm_finalize(s, GMM_FIN_EM, a);
    }
    DMVAE_LAUNCH(gmm_select_kernel, dim3(1), dim3(256), 0, s, a, *out);
    return check_launch(who);
}

}  // namespace dmvae
