// Exact t-SNE (van der Maaten & Hinton 2008; sklearn.manifold.TSNE(method="exact"), two output dimensions, alpha = 1) on the device.
// One dense [N][N] f32 buffer at the front of the caller's workspace holds, in turn and in place, the squared distances, the
// conditional p_{j|i} and the joint P.  Every pass over it gives a row to ONE wave (four rows per workgroup): the lanes take the
// row's scalars in front of its first 16-byte boundary, then aligned float4s, then the scalars behind the last one (tsne_row_visit:
// a row starts at element i * N, which is aligned for no N that is odd), and the wave's sums are xor-butterflies of a fixed order.
// Nothing is kept in LDS per row, so no N has to fit anywhere: the perplexity search re-reads its row (L1 / L2) at every step.
//   tsne_d2_kernel          d2_ij = sum_d (x_id - x_jd)^2, f32 differences, d ascending; 16 x 256 tiles, X staged in LDS 32 columns at a time
//   tsne_perplexity_kernel  row minimum over j != i, 64 bisection steps on beta (no early exit) with s and the entropy's numerator in
//                           f64, one more pass for s at the final beta, then p_{j|i} = exp(-beta d') / s over the row, p_{i|i} = 0
//   tsne_symmetrize_kernel  64 x 64 tile pairs (ty <= tx): P_ij = (p_{j|i} + p_{i|j}) / 2N formed ONCE per unordered pair and stored to both
//                           places through LDS, so both stores are row-contiguous and P == P^T bit for bit
// and per iteration, three launches:
//   tsne_pairs_kernel       row i: sum_j P_ij q_ij (y_i - y_j), sum_j q_ij^2 (y_i - y_j), sum_j q_ij (q = 1 / (1 + |y_i - y_j|^2), q_ii = 0)
//   tsne_sum_kernel         Z = sum_i of the rows' shares in f64: a thread adds a contiguous stretch in order, thread 0 the 256 stretches in order
//   tsne_update_kernel      g = 4 (e attr - rep / Z), then sklearn's gains / momentum update (tsne_grad_kernel: g alone)
// The KL divergence reuses the first two at the final Y, then tsne_kl_kernel (f64 terms, one partial per workgroup) and tsne_sum_kernel.
// No float atomics and no host synchronisation anywhere: every launch of a fit is enqueued up front, and two runs agree bit for bit.
#include <math.h>

#include "tsne.h"

namespace dmvae {

struct TsneWs {
    float* P;           // [N][N] d2, then p_{j|i}, then the joint P
    float* beta;        // [N]
    float4* acc;        // [N] {attr_x, attr_y, rep_x, rep_y}
    double* zrow;       // [N] sum_j q_ij
    double* Z;          // [1]
    float* U;           // [N][2] the fit's velocity
    float* G;           // [N][2] the fit's gains
    double* klpart;     // [ceil(N / 4)]
};

__device__ __forceinline__ double tsne_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// scalars of row i in front of its first 16-byte boundary (the buffer itself is 16-byte aligned)
__device__ __forceinline__ int tsne_row_head(int i, int N) { return (int)((4 - (((int64_t)i * N) & 3)) & 3); }

// f(j, v) for every element j of the row, dealt to the wave's 64 lanes; WRITE: f returns the value stored back
template <bool WRITE, class F>
__device__ __forceinline__ void tsne_row_visit(float* row, int N, int head, int lane, F&& f) {
    if (lane < head) {
        if constexpr (WRITE) row[lane] = f(lane, row[lane]); else f(lane, row[lane]);
    }
    const int nvec = (N - head) >> 2;
    float4* rv = reinterpret_cast<float4*>(row + head);
    for (int v = lane; v < nvec; v += 64) {
        float4 x = rv[v];
        const int j = head + 4 * v;
        if constexpr (WRITE) {
            x.x = f(j, x.x); x.y = f(j + 1, x.y); x.z = f(j + 2, x.z); x.w = f(j + 3, x.w);
            rv[v] = x;
        } else {
            f(j, x.x); f(j + 1, x.y); f(j + 2, x.z); f(j + 3, x.w);
        }
    }
    const int t = head + 4 * nvec + lane;
    if (t < N) {
        if constexpr (WRITE) row[t] = f(t, row[t]); else f(t, row[t]);
    }
}

constexpr int D2_ROWS = 16, D2_COLS = 256, D2_DC = 32;

__global__ __launch_bounds__(256) void tsne_d2_kernel(int N, int D, const float* __restrict__ X, int64_t ldx, float* __restrict__ P) {
    __shared__ float xi[D2_ROWS][D2_DC];
    __shared__ float xj[D2_COLS][D2_DC + 1];
    const int tid = threadIdx.x, j0 = blockIdx.x * D2_COLS, i0 = blockIdx.y * D2_ROWS;
    float acc[D2_ROWS];
#pragma unroll
    for (int r = 0; r < D2_ROWS; ++r) acc[r] = 0.f;
    for (int d0 = 0; d0 < D; d0 += D2_DC) {
        for (int idx = tid; idx < D2_ROWS * D2_DC; idx += 256) {
            const int r = idx / D2_DC, c = idx % D2_DC;
            xi[r][c] = (i0 + r < N && d0 + c < D) ? X[(int64_t)(i0 + r) * ldx + d0 + c] : 0.f;
        }
        for (int idx = tid; idx < D2_COLS * D2_DC; idx += 256) {
            const int r = idx / D2_DC, c = idx % D2_DC;
            xj[r][c] = (j0 + r < N && d0 + c < D) ? X[(int64_t)(j0 + r) * ldx + d0 + c] : 0.f;
        }
        __syncthreads();
        const int dn = D - d0 < D2_DC ? D - d0 : D2_DC;
        for (int d = 0; d < dn; ++d) {
            const float v = xj[tid][d];
#pragma unroll
            for (int r = 0; r < D2_ROWS; ++r) {
                const float df = xi[r][d] - v;
                acc[r] += df * df;
            }
        }
        __syncthreads();
    }
    const int j = j0 + tid;
    if (j < N) {
#pragma unroll
        for (int r = 0; r < D2_ROWS; ++r)
            if (i0 + r < N) P[(int64_t)(i0 + r) * N + j] = acc[r];
    }
}

__global__ __launch_bounds__(256) void tsne_perplexity_kernel(int N, float perplexity, float* __restrict__ P, float* __restrict__ beta_out) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                        // (no barrier in this kernel)
    float* row = P + (int64_t)i * N;
    const int head = tsne_row_head(i, N);
    float mn = INFINITY;
    tsne_row_visit<false>(row, N, head, lane, [&](int j, float v) { if (j != i) mn = fminf(mn, v); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
    const double target = log((double)perplexity);
    float beta = 1.f, lo = 0.f, hi = 0.f;                      // lo = 0: (beta + lo) / 2 halves while no lower bound is known
    bool has_hi = false;
    double s = 1.0;
    for (int step = 0; step <= TSNE_SEARCH_STEPS; ++step) {    // the last trip only takes s at the final beta
        double ls = 0.0, ln = 0.0;
        tsne_row_visit<false>(row, N, head, lane, [&](int j, float v) {
            if (j != i) {
                const float d = v - mn, e = expf(-beta * d);
                ls += (double)e;
                ln += (double)(d * e);
            }
        });
        s = tsne_wave_sum(ls);                                 // >= 1: the row's minimum contributes exp(0)
        if (step == TSNE_SEARCH_STEPS) break;
        const double H = log(s) + (double)beta * tsne_wave_sum(ln) / s;
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
    tsne_row_visit<true>(row, N, head, lane, [&](int j, float v) { return j == i ? 0.f : expf(-beta * (v - mn)) * inv_s; });
    if (lane == 0) beta_out[i] = beta;
}

__global__ __launch_bounds__(256) void tsne_symmetrize_kernel(int N, float* __restrict__ P) {
    __shared__ float sa[64][65], sb[64][65];
    const int tx = blockIdx.x, ty = blockIdx.y, tid = threadIdx.x;
    if (ty > tx) return;
    const bool diag = tx == ty;
    const int r0 = ty * 64, c0 = tx * 64;
    const float two_n = 2.f * (float)N;
    for (int idx = tid; idx < 4096; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        sa[r][c] = (r0 + r < N && c0 + c < N) ? P[(int64_t)(r0 + r) * N + c0 + c] : 0.f;
        if (!diag) sb[r][c] = (c0 + r < N && r0 + c < N) ? P[(int64_t)(c0 + r) * N + r0 + c] : 0.f;
    }
    __syncthreads();
    // element (r, c) of the tile pairs with (c, r) of the mirrored tile: one thread forms the pair's value and leaves it in both
    for (int idx = tid; idx < 4096; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        if (diag) {
            if (c >= r) {
                const float v = (sa[r][c] + sa[c][r]) / two_n;
                sa[r][c] = v;
                sa[c][r] = v;
            }
        } else {
            const float v = (sa[r][c] + sb[c][r]) / two_n;
            sa[r][c] = v;
            sb[c][r] = v;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < 4096; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        if (r0 + r < N && c0 + c < N) P[(int64_t)(r0 + r) * N + c0 + c] = sa[r][c];
        if (!diag && c0 + r < N && r0 + c < N) P[(int64_t)(c0 + r) * N + r0 + c] = sb[r][c];
    }
}

__global__ __launch_bounds__(256) void tsne_pairs_kernel(int N, const float* __restrict__ P, const float* __restrict__ Y, float4* __restrict__ acc,
                                                         double* __restrict__ zrow) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                        // (no barrier in this kernel)
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    const float2 yi = Y2[i];
    float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f;
    tsne_row_visit<false>(const_cast<float*>(P) + (int64_t)i * N, N, tsne_row_head(i, N), lane, [&](int j, float p) {
        const float2 yj = Y2[j];
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float q = j == i ? 0.f : __builtin_amdgcn_rcpf(1.f + dx * dx + dy * dy);
        const float pq = p * q, qq = q * q;
        ax += pq * dx; ay += pq * dy;
        rx += qq * dx; ry += qq * dy;
        z += q;
    });
    ax = wave_sum(ax); ay = wave_sum(ay); rx = wave_sum(rx); ry = wave_sum(ry);
    const double zd = tsne_wave_sum((double)z);
    if (lane == 0) {
        acc[i] = make_float4(ax, ay, rx, ry);
        zrow[i] = zd;
    }
}

// out[0] = in[0] + in[1] + ... in a fixed order: thread t adds its contiguous stretch, thread 0 the 256 stretches; one workgroup
__global__ __launch_bounds__(256) void tsne_sum_kernel(const double* __restrict__ in, int n, double* __restrict__ out) {
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

__device__ __forceinline__ float2 tsne_grad_of(const float4 a, double Z, float e) {
    const double inv_z = 1.0 / Z;
    return make_float2((float)(4.0 * ((double)e * a.x - a.z * inv_z)), (float)(4.0 * ((double)e * a.y - a.w * inv_z)));
}

__global__ __launch_bounds__(256) void tsne_grad_kernel(int N, const float4* __restrict__ acc, const double* __restrict__ Z, float e, float* __restrict__ grad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) reinterpret_cast<float2*>(grad)[i] = tsne_grad_of(acc[i], Z[0], e);
}

// sklearn's _gradient_descent, one element: every product and sum rounded on its own
__device__ __forceinline__ void tsne_update_elem(float& y, float& u, float& gn, float g, float m, float lr) {
#pragma clang fp contract(off)
    const bool inc = u * g < 0.f;
    gn = inc ? gn + 0.2f : gn * 0.8f;
    gn = fmaxf(gn, 0.01f);
    const float mu = m * u, step = lr * (gn * g);
    u = mu - step;
    y = y + u;
}

__global__ __launch_bounds__(256) void tsne_update_kernel(int N, const float4* __restrict__ acc, const double* __restrict__ Z, float e, float m, float lr,
                                                          float* __restrict__ Y, float* __restrict__ U, float* __restrict__ G) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float2 g = tsne_grad_of(acc[i], Z[0], e);
    float2 y = reinterpret_cast<float2*>(Y)[i], u = reinterpret_cast<float2*>(U)[i], gn = reinterpret_cast<float2*>(G)[i];
    tsne_update_elem(y.x, u.x, gn.x, g.x, m, lr);
    tsne_update_elem(y.y, u.y, gn.y, g.y, m, lr);
    reinterpret_cast<float2*>(Y)[i] = y;
    reinterpret_cast<float2*>(U)[i] = u;
    reinterpret_cast<float2*>(G)[i] = gn;
}

// Y = Y0, or 1e-4 * the Philox normals; U = 0, G = 1
__global__ __launch_bounds__(256) void tsne_init_kernel(int n2, const float* Y0, uint64_t seed, float* Y, float* __restrict__ U,
                                                        float* __restrict__ G) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n2) return;
    Y[k] = Y0 ? Y0[k] : 1e-4f * philox_normal_at(seed, 0, TSNE_PHILOX_STREAM, (uint64_t)k);
    U[k] = 0.f;
    G[k] = 1.f;
}

// sum over P_ij > 0 of P_ij log(P_ij Z (1 + |y_i - y_j|^2)), f64 terms: one partial per workgroup (four rows)
__global__ __launch_bounds__(256) void tsne_kl_kernel(int N, const float* __restrict__ P, const float* __restrict__ Y, const double* __restrict__ Zp,
                                                      double* __restrict__ part) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * 4 + w;
    double t = 0.0;
    if (i < N) {
        const float2* Y2 = reinterpret_cast<const float2*>(Y);
        const float2 yi = Y2[i];
        const double Z = Zp[0];
        tsne_row_visit<false>(const_cast<float*>(P) + (int64_t)i * N, N, tsne_row_head(i, N), lane, [&](int j, float p) {
            if (p > 0.f) {
                const float2 yj = Y2[j];
                const float dx = yi.x - yj.x, dy = yi.y - yj.y;
                t += (double)p * log((double)p * Z * (double)(1.f + dx * dx + dy * dy));
            }
        });
    }
    t = tsne_wave_sum(t);
    if (lane == 0) red[w] = t;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------------------------- host side
int tsne_check(const dmvae_tsne_config* c, const char* who) {
    if (!c) {
        set_error("%s: null config", who);
        return DMVAE_EINVAL;
    }
    if (c->N < 4 || c->D < 1 || !(c->perplexity > 1.f) || !(c->perplexity < (float)(c->N - 1)) || c->n_iter < 0 || c->exaggeration_iters < 0 ||
        c->flags != 0 || !(c->early_exaggeration > 0.f) || !(c->learning_rate > 0.f)) {
        set_error("%s: needs N >= 4, D >= 1, 1 < perplexity < N - 1, n_iter >= 0, exaggeration_iters >= 0, early_exaggeration > 0, learning_rate > 0 "
                  "and flags 0; got N=%d D=%d perplexity=%g n_iter=%d exaggeration_iters=%d early_exaggeration=%g learning_rate=%g flags=%d", who, c->N,
                  c->D, (double)c->perplexity, c->n_iter, c->exaggeration_iters, (double)c->early_exaggeration, (double)c->learning_rate, c->flags);
        return DMVAE_EINVAL;
    }
    if (c->N > TSNE_MAX_N) {
        set_error("%s: N=%d is above %d (the dense N x N f32 matrix would pass 4 GiB)", who, c->N, TSNE_MAX_N);
        return DMVAE_EUNSUPPORTED;
    }
    return 0;
}

static int64_t tsne_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// the workspace's arrays, in order (P first: dmvae_tsne_p is the workspace's own address); base == nullptr: only the total
static int64_t tsne_carve(const dmvae_tsne_config* c, char* base, TsneWs* w) {
    const int64_t N = c->N;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += tsne_up256(bytes); return p; };
    TsneWs t;
    t.P = (float*)take(N * N * 4);
    t.beta = (float*)take(N * 4);
    t.acc = (float4*)take(N * 16);
    t.zrow = (double*)take(N * 8);
    t.Z = (double*)take(8);
    t.U = (float*)take(N * 8);
    t.G = (float*)take(N * 8);
    t.klpart = (double*)take((N + 3) / 4 * 8);
    if (w) *w = t;
    return off;
}

int64_t tsne_ws_bytes(const dmvae_tsne_config* c) { return tsne_carve(c, nullptr, nullptr); }

static int tsne_ws_check(const dmvae_tsne_config* c, const void* ws, int64_t ws_bytes, const char* who) {
    if (!ws || ws_bytes < tsne_ws_bytes(c) || ((uintptr_t)ws & 15)) {
        set_error("%s: the workspace needs %lld bytes (dmvae_tsne_ws_bytes), 16-byte aligned; got %lld at %p", who, (long long)tsne_ws_bytes(c),
                  (long long)ws_bytes, ws);
        return DMVAE_EINVAL;
    }
    return 0;
}

static int tsne_rows_grid(int N) { return (N + 3) / 4; }

// steps 1-3 into w.P (arguments checked by the caller)
static void tsne_joint_p_enqueue(hipStream_t s, const dmvae_tsne_config* c, const float* X, int64_t ldx, const TsneWs& w, float* beta) {
    const int N = c->N;
    const double n2 = (double)N * N;
    ProfScope ps(s, "tsne_joint_p", n2 * (3.0 * c->D + 12.0 * (TSNE_SEARCH_STEPS + 2)), n2 * 4.0 * 6.0);
    DMVAE_LAUNCH(tsne_d2_kernel, dim3((N + D2_COLS - 1) / D2_COLS, (N + D2_ROWS - 1) / D2_ROWS), dim3(256), 0, s, N, c->D, X, ldx, w.P);
    DMVAE_LAUNCH(tsne_perplexity_kernel, dim3(tsne_rows_grid(N)), dim3(256), 0, s, N, c->perplexity, w.P, beta ? beta : w.beta);
    const int T = (N + 63) / 64;
    DMVAE_LAUNCH(tsne_symmetrize_kernel, dim3(T, T), dim3(256), 0, s, N, w.P);
}

// the rows' attractive / repulsive sums and Z at Y: two launches
static void tsne_pairs_enqueue(hipStream_t s, int N, const TsneWs& w, const float* Y) {
    DMVAE_LAUNCH(tsne_pairs_kernel, dim3(tsne_rows_grid(N)), dim3(256), 0, s, N, w.P, Y, w.acc, w.zrow);
    DMVAE_LAUNCH(tsne_sum_kernel, dim3(1), dim3(256), 0, s, w.zrow, N, w.Z);
}

// one iteration: three launches (dmvae_tsne_step and every iteration of dmvae_tsne_fit)
static void tsne_step_enqueue(hipStream_t s, const dmvae_tsne_config* c, const TsneWs& w, float* Y, float* U, float* G, float e, float m) {
    const int N = c->N;
    ProfScope ps(s, "tsne_step", (double)N * N * 14.0, (double)N * N * 4.0);
    tsne_pairs_enqueue(s, N, w, Y);
    DMVAE_LAUNCH(tsne_update_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, w.acc, w.Z, e, m, c->learning_rate, Y, U, G);
}

int tsne_joint_p_launch(hipStream_t s, const dmvae_tsne_config* c, const float* X, int64_t ldx, void* ws, int64_t ws_bytes, float* beta) {
    const char* who = "dmvae_tsne_joint_p";
    if (int rc = tsne_check(c, who)) return rc;
    if (!X || ldx < c->D) {
        set_error("%s: X must be given and ldx >= D", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneWs w;
    tsne_carve(c, (char*)ws, &w);
    tsne_joint_p_enqueue(s, c, X, ldx, w, beta);
    return check_launch(who);
}

int tsne_gradient_launch(hipStream_t s, const dmvae_tsne_config* c, void* ws, int64_t ws_bytes, const float* Y, float exaggeration, float* grad) {
    const char* who = "dmvae_tsne_gradient";
    if (int rc = tsne_check(c, who)) return rc;
    if (!Y || !grad || ((uintptr_t)Y & 7) || ((uintptr_t)grad & 7)) {
        set_error("%s: Y and grad must be given, 8-byte aligned", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneWs w;
    tsne_carve(c, (char*)ws, &w);
    tsne_pairs_enqueue(s, c->N, w, Y);
    DMVAE_LAUNCH(tsne_grad_kernel, dim3((c->N + 255) / 256), dim3(256), 0, s, c->N, w.acc, w.Z, exaggeration, grad);
    return check_launch(who);
}

int tsne_step_launch(hipStream_t s, const dmvae_tsne_config* c, void* ws, int64_t ws_bytes, float* Y, float* U, float* G, float exaggeration,
                     float momentum) {
    const char* who = "dmvae_tsne_step";
    if (int rc = tsne_check(c, who)) return rc;
    if (!Y || !U || !G || (((uintptr_t)Y | (uintptr_t)U | (uintptr_t)G) & 7)) {
        set_error("%s: Y, U and G must be given, 8-byte aligned", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneWs w;
    tsne_carve(c, (char*)ws, &w);
    tsne_step_enqueue(s, c, w, Y, U, G, exaggeration, momentum);
    return check_launch(who);
}

int tsne_fit_launch(hipStream_t s, const dmvae_tsne_config* c, const float* X, int64_t ldx, const float* Y0, void* ws, int64_t ws_bytes, float* Y,
                    double* kl) {
    const char* who = "dmvae_tsne_fit";
    if (int rc = tsne_check(c, who)) return rc;
    if (!X || ldx < c->D || !Y || !kl || ((uintptr_t)Y & 7) || ((uintptr_t)kl & 7)) {
        set_error("%s: X, Y, kl must be given (Y and kl 8-byte aligned) and ldx >= D", who);
        return DMVAE_EINVAL;
    }
    if (int rc = tsne_ws_check(c, ws, ws_bytes, who)) return rc;
    TsneWs w;
    tsne_carve(c, (char*)ws, &w);
    const int N = c->N;
    tsne_joint_p_enqueue(s, c, X, ldx, w, nullptr);
    DMVAE_LAUNCH(tsne_init_kernel, dim3((2 * N + 255) / 256), dim3(256), 0, s, 2 * N, Y0, c->seed, Y, w.U, w.G);
    for (int it = 0; it < c->n_iter; ++it) {
        const bool early = it < c->exaggeration_iters;
        tsne_step_enqueue(s, c, w, Y, w.U, w.G, early ? c->early_exaggeration : 1.f, early ? 0.5f : 0.8f);
    }
    tsne_pairs_enqueue(s, N, w, Y);
    DMVAE_LAUNCH(tsne_kl_kernel, dim3(tsne_rows_grid(N)), dim3(256), 0, s, N, w.P, Y, w.Z, w.klpart);
    DMVAE_LAUNCH(tsne_sum_kernel, dim3(1), dim3(256), 0, s, w.klpart, tsne_rows_grid(N), kl);
    return check_launch(who);
}

}  // namespace dmvae
