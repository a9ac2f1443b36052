// Cluster quality on the device: the label of every row and the silhouette coefficient (Rousseeuw 1987;
// sklearn.metrics.silhouette_samples with the Euclidean metric) of rows Z [n][ldz] under int32 labels in [0, K).
//   n_k  = rows with label k
//   d_ij = sqrt(sum_c (z_ic - z_jc)^2)                     f32 DIFFERENCES, c ascending (no norm expansion: near rows do not cancel)
//   a_i  = sum_{j: l_j = l_i} d_ij / (n_{l_i} - 1)         (d_ii = 0 exactly, so the row itself may stay in the sum)
//   b_i  = min over k != l_i with n_k > 0 of sum_{j: l_j = k} d_ij / n_k
//   s_i  = (b_i - a_i) / max(a_i, b_i);   0 when n_{l_i} = 1, when max(a_i, b_i) = 0 or when no other cluster has a row
// No N x N and no N x K array is stored.  The columns are grouped by label first, so that a column tile belongs to one cluster:
//   argmax_labels_kernel  16 lanes per row: labels[r] = first index of the row's largest score (row_argmax.h)
//   sil_hist_kernel       n_k by integer atomics (exact in any order); a label outside [0, K) sets the error flag and counts nowhere
//   sil_scan_kernel       one workgroup: exclusive scan of the n_k, and out[1] = the number of non-empty clusters
//   sil_group_kernel      one workgroup per non-empty cluster: its row indices in ASCENDING order behind the cluster's offset.  Each
//                         wave takes one contiguous stretch of the label array, counts its matches, and after one barrier compacts
//                         them by ballot and prefix -- a stable grouping, where a scatter by atomics would order a cluster (and so
//                         round the f32 sums) differently from run to run
//   sil_pairs_kernel      a workgroup owns 16 rows and walks every cluster's column tiles (256 columns, one per thread; the last tile
//                         of a cluster is masked).  Z passes through LDS 32 columns of D at a time; a thread keeps the 16 squared
//                         distances of its column in registers across the chunks, takes the correctly rounded sqrtf, and adds into
//                         16 f32 running sums.  A running sum takes at most 64 distances before it is added into the thread's
//                         double; at the end of a cluster the doubles of the 256 threads are added in a fixed order (xor butterfly,
//                         then the four waves in order) and thread r < 16 forms a / the running min of b for row r in double
//   sil_sum_kernel        out[0] = sum_i s_i in double: a thread adds a contiguous stretch in order, thread 0 the 256 stretches
// No float atomics, every sum in a fixed order: two calls on the same inputs return the same bits.
#include <math.h>

#include "cluster_metrics.h"
#include "row_argmax.h"

namespace dmvae {

constexpr int SIL_ROWS = 16, SIL_COLS = 256, SIL_DC = 32;
constexpr int SIL_LDJ = SIL_DC + 4;              // row stride of the column tile in LDS: 16-byte reads of 16 lanes fall into 64 distinct banks
constexpr int SIL_FLUSH = 64;                    // distances a running f32 sum takes before it goes into the double
constexpr int SIL_GROUP_WAVES = 8;

struct SilWs {
    int32_t* counts;    // [K] n_k
    int32_t* offs;      // [K] rows of the clusters before k
    int32_t* sorted;    // [n] row indices grouped by label, ascending inside a cluster
    double* sd;         // [n] s_i
};

__global__ __launch_bounds__(256) void argmax_labels_kernel(const float* __restrict__ scores, int64_t ld, int n_valid, int K, int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = b < n_valid;
    const int bi = row_argmax16(scores + (int64_t)(valid ? b : 0) * ld, valid ? K : 0, lane);
    if (valid && lane == 0) labels[b] = bi;
}

__global__ __launch_bounds__(256) void sil_hist_kernel(const int32_t* __restrict__ labels, int n, int K, int32_t* counts, int32_t* err_flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = labels[i];
    if (l < 0 || l >= K) { atomicOr(err_flag, SIL_ERR_LABEL); return; }      // checked before it indexes anything
    atomicAdd(counts + l, 1);
}

__global__ __launch_bounds__(256) void sil_scan_kernel(const int32_t* __restrict__ counts, int K, int32_t* __restrict__ offs, double* __restrict__ out) {
    __shared__ int part[256], used[256];
    const int per = (K + 255) / 256, b = threadIdx.x * per;
    int s = 0, u = 0;
    for (int k = b; k < b + per && k < K; ++k) {
        const int c = counts[k];
        s += c;
        u += c > 0;
    }
    part[threadIdx.x] = s;
    used[threadIdx.x] = u;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0, nu = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
            nu += used[t];
        }
        out[1] = (double)nu;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int k = b; k < b + per && k < K; ++k) {
        offs[k] = run;
        run += counts[k];
    }
}

__global__ __launch_bounds__(64 * SIL_GROUP_WAVES) void sil_group_kernel(const int32_t* __restrict__ labels, int n, const int32_t* __restrict__ counts,
                                                                         const int32_t* __restrict__ offs, int32_t* __restrict__ sorted) {
    __shared__ int wcount[SIL_GROUP_WAVES];
    const int k = blockIdx.x;
    if (counts[k] == 0) return;                                  // (the whole workgroup)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int seg = (n + 64 * SIL_GROUP_WAVES - 1) / (64 * SIL_GROUP_WAVES) * 64;
    const int lo = w * seg, hi = lo + seg < n ? lo + seg : n;    // n <= 2^20: no overflow
    int c = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        c += __popcll(__ballot(i < hi && labels[i] == k));
    }
    if (lane == 0) wcount[w] = c;
    __syncthreads();
    int pos = offs[k];
    for (int v = 0; v < w; ++v) pos += wcount[v];
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool m = i < hi && labels[i] == k;
        const unsigned long long mask = __ballot(m);
        const int at = pos + __popcll(mask & ((1ull << lane) - 1ull));
        if (m && at < n) sorted[at] = i;                         // at < offs[k] + n_k <= n while the labels are what was counted
        pos += __popcll(mask);
    }
}

__device__ __forceinline__ double sil_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct SilArgs {
    const float* Z; int64_t ldz; int n, D, K;
    const int32_t* labels; const int32_t* counts; const int32_t* offs; const int32_t* sorted;
    float* samples; double* sd;
};

__global__ __launch_bounds__(256) void sil_pairs_kernel(SilArgs a) {
    __shared__ __attribute__((aligned(16))) float xi[SIL_ROWS][SIL_DC];
    __shared__ __attribute__((aligned(16))) float xj[SIL_COLS][SIL_LDJ];
    __shared__ int sidx[SIL_COLS];
    __shared__ double red[4][SIL_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i0 = blockIdx.x * SIL_ROWS;
    const int n = a.n, D = a.D, K = a.K;
    const int nchunk = (D + SIL_DC - 1) / SIL_DC;

    // thread r < SIL_ROWS keeps the scalars of row i0 + r
    int my_l = -1, my_n = 0;
    double my_a = 0.0, my_b = INFINITY;
    if (tid < SIL_ROWS && i0 + tid < n) {
        const int l = a.labels[i0 + tid];
        if (l >= 0 && l < K) { my_l = l; my_n = a.counts[l]; }
    }
    float fs[SIL_ROWS];
    double ds[SIL_ROWS];
#pragma unroll
    for (int r = 0; r < SIL_ROWS; ++r) { fs[r] = 0.f; ds[r] = 0.0; }
    bool xi_staged = false;                                      // D <= SIL_DC: the row tile is staged once for the whole walk

    for (int k = 0; k < K; ++k) {
        const int nk = a.counts[k];
        if (nk == 0) continue;                                   // (the whole workgroup)
        const int off = a.offs[k];
        int held = 0;
        for (int t0 = 0; t0 < nk; t0 += SIL_COLS) {
            const bool cv = t0 + tid < nk;                       // the cluster's last tile is ragged
            sidx[tid] = cv ? a.sorted[off + t0 + tid] : -1;
            float acc[SIL_ROWS];
#pragma unroll
            for (int r = 0; r < SIL_ROWS; ++r) acc[r] = 0.f;
            for (int ch = 0; ch < nchunk; ++ch) {
                const int d0 = ch * SIL_DC;
                const int dn = D - d0 < SIL_DC ? D - d0 : SIL_DC;
                const int dn4 = (dn + 3) & ~3;                   // columns dn .. dn4 are staged as zeros on both sides
                __syncthreads();                                 // sidx is written; the previous chunk's reads are done
                if (nchunk > 1 || !xi_staged) {
                    for (int idx = tid; idx < SIL_ROWS * SIL_DC; idx += 256) {
                        const int r = idx / SIL_DC, c = idx % SIL_DC;
                        xi[r][c] = (i0 + r < n && c < dn) ? a.Z[(int64_t)(i0 + r) * a.ldz + d0 + c] : 0.f;
                    }
                    xi_staged = true;
                }
                // idx / dn4 for idx < 8192 and dn4 <= 32 by one multiply: the error of the reciprocal stays below 8192 / 2^20 < 1 / 32
                const unsigned inv = ((1u << 20) + dn4 - 1) / dn4;
                for (int idx = tid; idx < SIL_COLS * dn4; idx += 256) {
                    const int r = (int)(((unsigned)idx * inv) >> 20), c = idx - r * dn4;
                    const int src = sidx[r];
                    xj[r][c] = (src >= 0 && src < n && c < dn) ? a.Z[(int64_t)src * a.ldz + d0 + c] : 0.f;
                }
                __syncthreads();
                for (int d = 0; d < dn4; d += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(&xj[tid][d]);
#pragma unroll
                    for (int r = 0; r < SIL_ROWS; ++r) {
                        const float4 u = *reinterpret_cast<const float4*>(&xi[r][d]);
                        const float e0 = u.x - v.x, e1 = u.y - v.y, e2 = u.z - v.z, e3 = u.w - v.w;
                        acc[r] += e0 * e0;
                        acc[r] += e1 * e1;
                        acc[r] += e2 * e2;
                        acc[r] += e3 * e3;
                    }
                }
            }
            if (cv) {
#pragma unroll
                for (int r = 0; r < SIL_ROWS; ++r) fs[r] += sqrtf(acc[r]);
            }
            if (++held == SIL_FLUSH) {
#pragma unroll
                for (int r = 0; r < SIL_ROWS; ++r) { ds[r] += (double)fs[r]; fs[r] = 0.f; }
                held = 0;
            }
        }
        // the cluster's sums over all of its columns, in double
#pragma unroll
        for (int r = 0; r < SIL_ROWS; ++r) {
            const double t = sil_wave_sum(ds[r] + (double)fs[r]);
            if (lane == 0) red[w][r] = t;
            ds[r] = 0.0;
            fs[r] = 0.f;
        }
        __syncthreads();                                         // (red is next written behind the next cluster's barriers)
        if (tid < SIL_ROWS && my_l >= 0) {
            const double S = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            if (k == my_l) my_a = my_n > 1 ? S / (double)(my_n - 1) : 0.0;
            else my_b = fmin(my_b, S / (double)nk);
        }
    }
    if (tid < SIL_ROWS && i0 + tid < n) {
        double s = 0.0;
        if (my_l >= 0 && my_n > 1 && my_b < (double)INFINITY) {
            const double m = fmax(my_a, my_b);
            if (m > 0.0) s = (my_b - my_a) / m;
        }
        a.sd[i0 + tid] = s;
        a.samples[i0 + tid] = (float)s;
    }
}

__global__ __launch_bounds__(256) void sil_sum_kernel(const double* __restrict__ in, int n, double* __restrict__ out) {
    __shared__ double part[256];
    const int chunk = (n + 255) / 256, b = threadIdx.x * chunk;
    double s = 0.0;
    for (int k = b; k < b + chunk && k < n; ++k) s += in[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += part[k];
        out[0] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define SIL_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int argmax_labels_launch(hipStream_t s, const float* scores, int64_t ld, int n_valid, int K, int32_t* labels) {
    const char* who = "dmvae_argmax_labels";
    SIL_REQUIRE(scores && labels, "%s: null scores / labels", who);
    SIL_REQUIRE(K >= 1 && K <= SIL_MAX_K && ld >= K, "%s: K=%d, ld=%lld (1 <= K <= %d, ld >= K)", who, K, (long long)ld, SIL_MAX_K);
    SIL_REQUIRE(n_valid >= 0, "%s: n_valid=%d", who, n_valid);
    if (n_valid == 0) return 0;
    ProfScope ps(s, "argmax_labels", (double)n_valid * K, 4.0 * n_valid * (K + 1.0));
    DMVAE_LAUNCH(argmax_labels_kernel, dim3((n_valid + 15) / 16), dim3(256), 0, s, scores, ld, n_valid, K, labels);
    return check_launch(who);
}

static int64_t sil_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

static int64_t sil_carve(int64_t n, int K, char* base, SilWs* w) {
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += sil_up256(bytes); return p; };
    SilWs t;
    t.counts = (int32_t*)take((int64_t)K * 4);
    t.offs = (int32_t*)take((int64_t)K * 4);
    t.sorted = (int32_t*)take(n * 4);
    t.sd = (double*)take(n * 8);
    if (w) *w = t;
    return off;
}

static int sil_shape_check(int64_t n, int K, const char* who) {
    SIL_REQUIRE(n >= 2 && n <= SIL_MAX_N && K >= 1 && K <= SIL_MAX_K, "%s: n=%lld, K=%d (2 <= n <= %d, 1 <= K <= %d)", who, (long long)n, K, SIL_MAX_N,
                SIL_MAX_K);
    return 0;
}

int64_t silhouette_ws_bytes(int64_t n, int K) {
    if (int rc = sil_shape_check(n, K, "dmvae_silhouette_ws_bytes")) return rc;
    return sil_carve(n, K, nullptr, nullptr);
}

int silhouette_launch(hipStream_t s, const float* Z, int64_t ldz, int n, int D, const int32_t* labels, int K, void* ws, int64_t ws_bytes, float* samples,
                      double* out, int32_t* err_flag) {
    const char* who = "dmvae_silhouette";
    if (int rc = sil_shape_check(n, K, who)) return rc;
    SIL_REQUIRE(Z && labels && samples && out && err_flag && ((uintptr_t)out & 7) == 0, "%s: Z, labels, samples, out (8-byte aligned) and err_flag must be given",
                who);
    SIL_REQUIRE(D >= 1 && ldz >= D, "%s: D=%d, ldz=%lld (D >= 1, ldz >= D)", who, D, (long long)ldz);
    const int64_t need = sil_carve(n, K, nullptr, nullptr);
    SIL_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "%s: the workspace needs %lld bytes (dmvae_silhouette_ws_bytes), 8-byte aligned; got %lld at %p",
                who, (long long)need, (long long)ws_bytes, ws);
    SilWs w;
    sil_carve(n, K, (char*)ws, &w);
    ProfScope ps(s, "silhouette", (double)n * n * (3.0 * D + 4.0), 4.0 * n * ((double)D * ((n + SIL_ROWS - 1) / SIL_ROWS) + 8.0));
    if (hipError_t e = hipMemsetAsync(w.counts, 0, (size_t)K * 4, s)) {
        set_error("%s: clearing the counts: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    DMVAE_LAUNCH(sil_hist_kernel, dim3((n + 255) / 256), dim3(256), 0, s, labels, n, K, w.counts, err_flag);
    DMVAE_LAUNCH(sil_scan_kernel, dim3(1), dim3(256), 0, s, w.counts, K, w.offs, out);
    DMVAE_LAUNCH(sil_group_kernel, dim3(K), dim3(64 * SIL_GROUP_WAVES), 0, s, labels, n, w.counts, w.offs, w.sorted);
    const SilArgs a{Z, ldz, n, D, K, labels, w.counts, w.offs, w.sorted, samples, w.sd};
    DMVAE_LAUNCH(sil_pairs_kernel, dim3((n + SIL_ROWS - 1) / SIL_ROWS), dim3(256), 0, s, a);
    DMVAE_LAUNCH(sil_sum_kernel, dim3(1), dim3(256), 0, s, w.sd, n, out);
    return check_launch(who);
}

}  // namespace dmvae
