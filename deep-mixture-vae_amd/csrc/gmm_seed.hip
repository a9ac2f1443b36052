// k-means++ seeding of the mixture fit's centres (Arthur & Vassilvitskii 2007; with T > 1 trials per centre the greedy form sklearn's
// GaussianMixture(init_params="kmeans") seeds with), n_init restarts side by side: the restart is blockIdx.y of every launch.
// State per restart in the workspace: d2 [N] f32 (squared distance to the nearest chosen centre), its per-workgroup sums [nblk] f64, every
// round's candidate rows [K][T], the chosen rows [K].  A row workgroup owns rpb = 256 * ceil(N / 65536) consecutive rows, so nblk <= 256 is a
// function of N alone and the partials fit one workgroup's scan.  Per centre k:
//   gmm_seed_select_kernel     grid (T, R): one workgroup per trial.  Thread b adds the f64 partials 0..b from LDS in block order (every thread
//                              the same serial order: prefix b has the bits a serial scan gives), tot = prefix nblk-1, target = u * tot; the
//                              block is the first with prefix > target (LDS integer atomicMin), and inside it thread t owns rpb / 256 consecutive
//                              rows: it loads them at once, adds them in f64, takes its exclusive prefix over the threads' sums the same way and
//                              walks its rows.  The row is the first with running sum > target and d2 > 0; rounding between the differently
//                              associated sums can leave no such row: then the last row with d2 > 0.  So one select costs three dependent
//                              trips (partials, the block's d2, the result), never one per row.  k = 0 or tot not > 0: min(floor(u N), N-1).
//   gmm_seed_potential_kernel  T > 1, k >= 1: the T candidate rows in LDS, one pass over X: sum_n min(d2_n, ||x_n - cand_t||^2) for all t at
//                              once as f64 partials [nblk][T].  Nothing of size [T][N] is written.
//   gmm_seed_commit_kernel     every workgroup adds the potentials' partials in block order and takes the smallest (first on ties), stages that
//                              row in LDS, sets d2 = min(d2, ||x - c_k||^2) (k = 0: the distance itself) and writes its new f64 partial;
//                              workgroup 0 writes the centre and its row index.
// Distances: differences in f32, summed over d in ascending order.  No float atomics, no host synchronisation: all K rounds are enqueued.
#include <limits.h>
#include <math.h>

#include "gmm_seed.h"

namespace dmvae {

struct SeedWs {
    int* cand;          // [R][K][T] candidate rows (round 0: trial 0, the others -1)
    float* d2;          // [R][N]
    double* part;       // [R][nblk] sums of d2
    double* potpart;    // [R][nblk][T] sums of min(d2, dist^2 to candidate t)
    int* idx;           // [R][K] chosen rows
};

struct SeedArgs {
    int N, D, K, R, T, nblk, rpt, k;      // rpt: rows per thread of a row workgroup; k: the round
    int64_t ldx;
    const float* X;
    const float* u;                       // [R][K][T] or null: Philox
    uint64_t seed;
    float* centers;                       // [R][K][D]
    int* rows;                            // [R][K] or null
    SeedWs ws;
};

// fixed-order sum over the 256 threads, valid in every thread
__device__ __forceinline__ double seed_block_sum(double v, double* red /* [4] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

__device__ __forceinline__ int seed_clamp_row(int row, int N) { return row < 0 ? 0 : (row >= N ? N - 1 : row); }

__global__ __launch_bounds__(256) void gmm_seed_select_kernel(SeedArgs a) {
    __shared__ double pp[256], pin[256];
    __shared__ int sh[4];                 // first block over the target, last block with a positive sum; the same for the rows
    const int r = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int64_t ui = ((int64_t)r * a.K + a.k) * a.T + t;
    const float u = a.u ? a.u[ui] : philox_uniform_at(a.seed, 0, GMM_SEED_PHILOX_STREAM, (uint64_t)ui);
    int* out = a.ws.cand + ui;
    const int64_t fr = (int64_t)((double)u * (double)N);
    const int uniform_row = (int)(fr < N - 1 ? fr : N - 1);
    if (a.k == 0) {
        if (tid == 0) *out = t == 0 ? uniform_row : -1;
        return;
    }
    pp[tid] = tid < a.nblk ? a.ws.part[(int64_t)r * a.nblk + tid] : 0.0;
    if (tid < 4) sh[tid] = (tid & 1) ? -1 : INT_MAX;
    __syncthreads();
    double incl = 0.0;
    for (int i = 0; i <= tid; ++i) incl += pp[i];         // threads past nblk add zeros: their prefix is the total
    pin[tid] = incl;
    __syncthreads();
    const double tot = pin[255];
    if (!(tot > 0.0)) {
        if (tid == 0) *out = uniform_row;
        return;
    }
    const double target = (double)u * tot;
    if (tid < a.nblk && pp[tid] > 0.0) {
        if (incl > target) atomicMin(&sh[0], tid);
        atomicMax(&sh[1], tid);
    }
    __syncthreads();
    const int B = sh[0] != INT_MAX ? sh[0] : sh[1];       // tot > 0: some block is positive
    const double base = B > 0 ? pin[B - 1] : 0.0;
    const int c = a.rpt;
    const int64_t my0 = ((int64_t)B * 256 + tid) * c;
    const float* d2r = a.ws.d2 + (int64_t)r * N;
    double loc = 0.0;
    for (int j = 0; j < c; ++j)
        if (my0 + j < N) loc += (double)d2r[my0 + j];
    pp[tid] = loc;                                        // (every read of the partials in pp is behind the barrier above)
    __syncthreads();
    double run = base;
    for (int i = 0; i < tid; ++i) run += pp[i];
    int first = INT_MAX, last = -1;
    for (int j = 0; j < c; ++j) {
        if (my0 + j >= N) break;
        const float v = d2r[my0 + j];
        run += (double)v;
        if (v > 0.f) {
            last = (int)(my0 + j);
            if (run > target && first == INT_MAX) first = last;
        }
    }
    if (first != INT_MAX) atomicMin(&sh[2], first);
    if (last >= 0) atomicMax(&sh[3], last);
    __syncthreads();
    if (tid == 0) *out = seed_clamp_row(sh[2] != INT_MAX ? sh[2] : sh[3], N);
}

template <int T>
__global__ __launch_bounds__(256) void gmm_seed_potential_kernel(SeedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    double* red = reinterpret_cast<double*>(lds);         // [4]
    float* crow = lds + 64;                               // [T][D] the candidates' rows
    const int r = blockIdx.y, tid = threadIdx.x, N = a.N, D = a.D;
    const int* cand = a.ws.cand + ((int64_t)r * a.K + a.k) * T;
    for (int idx = tid; idx < T * D; idx += 256) {
        const int t = idx / D, d = idx - t * D;
        crow[idx] = a.X[(int64_t)seed_clamp_row(cand[t], N) * a.ldx + d];
    }
    __syncthreads();
    double pot[T];
#pragma unroll
    for (int t = 0; t < T; ++t) pot[t] = 0.0;
    const float* d2r = a.ws.d2 + (int64_t)r * N;
    const int64_t row0 = (int64_t)blockIdx.x * 256 * a.rpt;
    for (int j = 0; j < a.rpt; ++j) {
        const int64_t n = row0 + tid + 256 * j;
        if (n >= N) break;
        const float* xr = a.X + n * a.ldx;
        float q[T];
#pragma unroll
        for (int t = 0; t < T; ++t) q[t] = 0.f;
        for (int d = 0; d < D; ++d) {
            const float x = xr[d];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float dx = x - crow[t * D + d];
                q[t] += dx * dx;
            }
        }
        const float old = d2r[n];
#pragma unroll
        for (int t = 0; t < T; ++t) pot[t] += (double)fminf(old, q[t]);
    }
    double* out = a.ws.potpart + ((int64_t)r * a.nblk + blockIdx.x) * T;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const double s = seed_block_sum(pot[t], red);
        if (tid == 0) out[t] = s;
    }
}

__global__ __launch_bounds__(256) void gmm_seed_commit_kernel(SeedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    double* red = reinterpret_cast<double*>(lds);         // [4] the sum's scratch, [4 .. 12) the trials' potentials
    int* swin = reinterpret_cast<int*>(red + 12);
    float* crow = lds + 64;                               // [D] the new centre
    const int r = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, N = a.N, D = a.D;
    const int Tk = a.k == 0 ? 1 : a.T;
    if (Tk > 1 && tid < Tk) {
        const double* pp = a.ws.potpart + (int64_t)r * a.nblk * a.T + tid;
        double s = 0.0;
        for (int i = 0; i < a.nblk; ++i) s += pp[(int64_t)i * a.T];
        red[4 + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int w = 0;
        for (int t = 1; t < Tk; ++t)
            if (red[4 + t] < red[4 + w]) w = t;           // strict: the first of equal potentials, as argmin
        *swin = w;
    }
    __syncthreads();
    const int64_t rk = (int64_t)r * a.K + a.k;
    const int row = seed_clamp_row(a.ws.cand[rk * a.T + *swin], N);
    const float* xc = a.X + (int64_t)row * a.ldx;
    for (int d = tid; d < D; d += 256) {
        const float v = xc[d];
        crow[d] = v;
        if (b == 0) a.centers[rk * D + d] = v;
    }
    if (b == 0 && tid == 0) {
        a.ws.idx[rk] = row;
        if (a.rows) a.rows[rk] = row;
    }
    __syncthreads();
    float* d2r = a.ws.d2 + (int64_t)r * N;
    const int64_t row0 = (int64_t)b * 256 * a.rpt;
    double acc = 0.0;
    for (int j = 0; j < a.rpt; ++j) {
        const int64_t n = row0 + tid + 256 * j;
        if (n >= N) break;
        const float* xr = a.X + n * a.ldx;
        float q = 0.f;
        for (int d = 0; d < D; ++d) {
            const float dx = xr[d] - crow[d];
            q += dx * dx;
        }
        const float nd = a.k == 0 ? q : fminf(d2r[n], q);
        d2r[n] = nd;
        acc += (double)nd;
    }
    const double s = seed_block_sum(acc, red);
    if (tid == 0) a.ws.part[(int64_t)r * a.nblk + b] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host side
int gmm_seed_trials(const dmvae_gmm_seed_config* c) { return c->local_trials ? c->local_trials : 2 + (int)log((double)c->K); }

static int seed_blocks(int N, int* rows_per_thread) {
    const int rpt = (int)(((int64_t)N + 65535) / 65536);
    *rows_per_thread = rpt;
    return (int)(((int64_t)N + 256 * (int64_t)rpt - 1) / (256 * (int64_t)rpt));
}

int gmm_seed_check(const dmvae_gmm_seed_config* c, const char* who) {
    if (!c || c->N < 1 || c->D < 1 || c->K < 1 || c->n_init < 1 || c->K > c->N || c->local_trials < 0 || c->local_trials > GMM_SEED_MAX_TRIALS ||
        c->flags != 0) {
        set_error("%s: N, D, K, n_init must be >= 1, K <= N, local_trials in 0..%d and flags 0", who, GMM_SEED_MAX_TRIALS);
        return DMVAE_EINVAL;
    }
    if ((int64_t)c->n_init * c->N > INT32_MAX || (int64_t)c->n_init * c->K * c->D > INT32_MAX || c->n_init > 65535) {
        set_error("%s: n_init * N and n_init * K * D must fit 31 bits, n_init <= 65535", who);
        return DMVAE_EINVAL;
    }
    const int T = gmm_seed_trials(c);
    const int64_t lb = (int64_t)4 * T * c->D + GMM_SEED_LDS_FIXED;
    if (T > GMM_SEED_MAX_TRIALS || lb > 65536) {
        set_error("%s: K=%d D=%d with %d trials needs trials <= %d (2 + int(ln K) when local_trials is 0) and 4 * trials * D + %d = %lld <= 65536 B of "
                  "LDS (the candidate rows live in LDS)", who, c->K, c->D, T, GMM_SEED_MAX_TRIALS, GMM_SEED_LDS_FIXED, (long long)lb);
        return DMVAE_EUNSUPPORTED;
    }
    return 0;
}

static int64_t seed_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// the workspace's arrays, in order (the candidates first: the header promises them there); base == nullptr: only the total
static int64_t seed_carve(const dmvae_gmm_seed_config* c, char* base, SeedWs* w) {
    int rpt;
    const int64_t R = c->n_init, K = c->K, T = gmm_seed_trials(c), nblk = seed_blocks(c->N, &rpt);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += seed_up256(bytes); return p; };
    SeedWs t;
    t.cand = (int*)take(R * K * T * 4);
    t.d2 = (float*)take(R * c->N * 4);
    t.part = (double*)take(R * nblk * 8);
    t.potpart = (double*)take(R * nblk * T * 8);
    t.idx = (int*)take(R * K * 4);
    if (w) *w = t;
    return off;
}

int64_t gmm_seed_ws_bytes(const dmvae_gmm_seed_config* c) { return seed_carve(c, nullptr, nullptr); }

template <int T>
static void seed_potential(hipStream_t s, const SeedArgs& a) {
    DMVAE_LAUNCH(gmm_seed_potential_kernel<T>, dim3(a.nblk, a.R), dim3(256), 256 + sizeof(float) * (size_t)T * a.D, s, a);
}

int gmm_seed_launch(hipStream_t s, const dmvae_gmm_seed_config* c, const float* X, int64_t ldx, const float* u, void* ws, int64_t ws_bytes,
                    float* centers, int32_t* rows) {
    const char* who = "dmvae_gmm_seed";
    if (int rc = gmm_seed_check(c, who)) return rc;
    if (!X || !ws || !centers || ldx < c->D) {
        set_error("%s: X, ws, centers must be given and ldx >= D", who);
        return DMVAE_EINVAL;
    }
    if (ws_bytes < gmm_seed_ws_bytes(c) || ((uintptr_t)ws & 7)) {
        set_error("%s: the workspace needs %lld bytes (dmvae_gmm_seed_ws_bytes), 8-byte aligned; got %lld", who, (long long)gmm_seed_ws_bytes(c),
                  (long long)ws_bytes);
        return DMVAE_EINVAL;
    }
    SeedArgs a{};
    a.N = c->N; a.D = c->D; a.K = c->K; a.R = c->n_init; a.T = gmm_seed_trials(c);
    a.nblk = seed_blocks(c->N, &a.rpt);
    a.ldx = ldx; a.X = X; a.u = u; a.seed = c->seed;
    a.centers = centers; a.rows = rows;
    seed_carve(c, (char*)ws, &a.ws);
    const double rows_all = (double)a.R * a.N * a.K;
    ProfScope ps(s, "gmm_seed", rows_all * a.D * 3.0 * (a.T > 1 ? a.T + 1 : 1), rows_all * (a.D + 2) * 4.0 * (a.T > 1 ? 2 : 1));
    for (int k = 0; k < a.K; ++k) {
        a.k = k;
        DMVAE_LAUNCH(gmm_seed_select_kernel, dim3(a.T, a.R), dim3(256), 0, s, a);
        if (k > 0 && a.T > 1) {
            switch (a.T) {
                case 2: seed_potential<2>(s, a); break;
                case 3: seed_potential<3>(s, a); break;
                case 4: seed_potential<4>(s, a); break;
                case 5: seed_potential<5>(s, a); break;
                case 6: seed_potential<6>(s, a); break;
                case 7: seed_potential<7>(s, a); break;
                default: seed_potential<8>(s, a); break;
            }
        }
        DMVAE_LAUNCH(gmm_seed_commit_kernel, dim3(a.nblk, a.R), dim3(256), 256 + sizeof(float) * (size_t)a.D, s, a);
    }
    return check_launch(who);
}

}  // namespace dmvae
