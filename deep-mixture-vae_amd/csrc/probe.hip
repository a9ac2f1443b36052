// Linear probe of the latent means on the device: ONE evaluation of the multinomial logistic regression loss and its gradient over all
// n rows (the hot path of an L-BFGS fit, dmvae_hip/probe.py), and the scores of a fitted probe.  Definitions (include/dmvae_hip.h):
//   x_id = (Z_id - shift_d) * scale_d in f32 (Z bit for bit without shift / scale);   l_ic = b_c, then fmaf(x_id, W_dc, l_ic), d ascending;
//   m_i = max_c l_ic;  s_i = sum_c exp(l_ic - m_i);  loss_i = log s_i + m_i - l_iy (finite when p_iy underflows);  r_ic = exp(l_ic - m_i) / s_i - [c = y_i]
//   probe_xent_kernel    a 256-thread workgroup owns a slab of 32-row tiles.  W and b sit in LDS for the whole slab as W' [D + 1][C4] (row D
//                        is b, the columns C .. C4 are zero), a tile's x rows as X' [32][Dp] (column D is 1 for a valid row: the bias
//                        gradient is row D of X'^T r; the columns above are zero).  Per tile: stage X'; logits in 4 rows x 4 classes per
//                        thread (two 16-byte LDS reads per four fmaf of a row block); softmax by 16 lanes per row, which leaves r in place
//                        of the logits and adds loss_i to the f64 sum of the row's first lane; then every thread adds x_id r_ic of the 32
//                        rows, ascending, to the (d, c) entries it owns for the whole slab -- a strip of ND columns d by 4 classes, f64
//                        registers (the product of two f32 is exact there; at an optimum the sums are small against their terms),
//                        again two 16-byte reads per 16 fma.  The slab's sums go to the workspace: no atomics on floats.
//   probe_finalize_kernel  the workgroups' f64 partials are added in a fixed order (16 groups of ascending workgroups per column, then
//                        the groups ascending) and divided by n.
//   probe_scores_kernel  the same W', X' and logits function; the 4 x 4 blocks go to global memory instead of LDS.
// The grid, the slabs and with them the order of every addition are functions of (n, D, C) alone: two calls return the same bits.
#include "probe.h"

namespace dmvae {

constexpr int PROBE_TR = 32;                     // rows of a tile
constexpr int PROBE_MAX_WG = 1024;

struct ProbeGeom {
    int C4, Dp, LDR;                             // classes and D + 1 columns rounded up to 4; row stride of the logits / r tile
    int G, ND;                                   // class blocks of 4 x G thread groups <= 256 threads; a group's strip of ND columns of X'
    int tiles, tiles_per_wg, nwg;
    size_t w_floats, lds_bytes;
};

struct ProbeArgs {
    const float* Z; int64_t ldz; int64_t n; int D, C;
    const float* shift; const float* scale; const int32_t* classes;
    const float* W; int64_t ldw; const float* b;
    ProbeGeom g;
    double* part; double* lossp; int32_t* flag;  // the loss kernel: [nwg][(D + 1) C] and [nwg]
    float* scores; int64_t lds;                  // the scores kernel
};

// W' [D + 1][C4] in LDS: rows d < D hold W, row D holds b, the columns C .. C4 hold zeros
__device__ __forceinline__ void probe_stage_w(float* sW, const ProbeArgs& a) {
    const int C4 = a.g.C4, total = (a.D + 1) * C4;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int d = idx / C4, c = idx - d * C4;
        sW[idx] = c < a.C ? (d < a.D ? a.W[(int64_t)d * a.ldw + c] : a.b[c]) : 0.f;
    }
}

// X' [32][Dp] in LDS for the rows row0 .. row0 + 32: x_id = (Z_id - shift_d) * scale_d, column D = 1, the columns above and the rows >= n zero.
// One wave per row: 256 contiguous bytes of Z per load.
__device__ __forceinline__ void probe_stage_x(float* sX, const ProbeArgs& a, int64_t row0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, Dp = a.g.Dp, D = a.D;
    for (int i = w; i < PROBE_TR; i += 4) {
        const int64_t row = row0 + i;
        const bool valid = row < a.n;
        const float* z = a.Z + row * a.ldz;
        for (int d = lane; d < Dp; d += 64) {
            float v = 0.f;
            if (valid) {
                if (d < D) {
                    v = z[d];
                    if (a.shift) v = (v - a.shift[d]) * a.scale[d];
                } else if (d == D) {
                    v = 1.f;
                }
            }
            sX[i * Dp + d] = v;
        }
    }
}

// l_ic for the tile in LDS: thread (g, cb) owns the classes 4 cb .. 4 cb + 3 of the row blocks g, g + G, ..; store(i, c0, l[4]) takes row i's four
__device__ __forceinline__ void probe_fma4(float (&acc)[4], float x, const float4& w) {
    acc[0] = fmaf(x, w.x, acc[0]); acc[1] = fmaf(x, w.y, acc[1]); acc[2] = fmaf(x, w.z, acc[2]); acc[3] = fmaf(x, w.w, acc[3]);
}
// the gradient's terms: the product of two f32 is exact in f64
__device__ __forceinline__ void probe_fma4d(double (&acc)[4], float x, const double (&r)[4]) {
    const double xd = (double)x;
    acc[0] = fma(xd, r[0], acc[0]); acc[1] = fma(xd, r[1], acc[1]); acc[2] = fma(xd, r[2], acc[2]); acc[3] = fma(xd, r[3], acc[3]);
}
template <class Store>
__device__ __forceinline__ void probe_logits(const float* sW, const float* sX, const ProbeArgs& a, Store store) {
    const int C4 = a.g.C4, Dp = a.g.Dp, D = a.D, CB4 = C4 >> 2;
    const int g = threadIdx.x / CB4, c0 = (threadIdx.x - g * CB4) * 4;
    if (g >= a.g.G) return;
    const float4 bias = *reinterpret_cast<const float4*>(&sW[D * C4 + c0]);
    const int D4 = D & ~3;
    for (int rb = g; rb * 4 < PROBE_TR; rb += a.g.G) {
        const float* x0 = sX + rb * 4 * Dp;
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[r][0] = bias.x; acc[r][1] = bias.y; acc[r][2] = bias.z; acc[r][3] = bias.w; }
        for (int d = 0; d < D4; d += 4) {
            float4 xv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) xv[r] = *reinterpret_cast<const float4*>(&x0[r * Dp + d]);
            const float4 w0 = *reinterpret_cast<const float4*>(&sW[(d + 0) * C4 + c0]);
            const float4 w1 = *reinterpret_cast<const float4*>(&sW[(d + 1) * C4 + c0]);
            const float4 w2 = *reinterpret_cast<const float4*>(&sW[(d + 2) * C4 + c0]);
            const float4 w3 = *reinterpret_cast<const float4*>(&sW[(d + 3) * C4 + c0]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                probe_fma4(acc[r], xv[r].x, w0); probe_fma4(acc[r], xv[r].y, w1); probe_fma4(acc[r], xv[r].z, w2); probe_fma4(acc[r], xv[r].w, w3);
            }
        }
        for (int d = D4; d < D; ++d) {
            const float4 w0 = *reinterpret_cast<const float4*>(&sW[d * C4 + c0]);
#pragma unroll
            for (int r = 0; r < 4; ++r) probe_fma4(acc[r], x0[r * Dp + d], w0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) store(rb * 4 + r, c0, acc[r]);
    }
}

template <int NDT>
__global__ __launch_bounds__(256) void probe_xent_kernel(ProbeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float probe_smem[];
    __shared__ double red[16];
    const int tid = threadIdx.x, C = a.C, C4 = a.g.C4, Dp = a.g.Dp, LDR = a.g.LDR, ND = a.g.ND, CB4 = C4 >> 2;
    float* sW = probe_smem;
    float* sX = sW + a.g.w_floats;
    float* sR = sX + PROBE_TR * Dp;
    probe_stage_w(sW, a);

    const int gg = tid / CB4, c0 = (tid - gg * CB4) * 4, d0 = gg * ND;   // the gradient entries of this thread: d0 .. d0 + ND by c0 .. c0 + 3
    const bool owner = gg < a.g.G && d0 < Dp;
    double acc[NDT][4];                                          // f64: at an optimum the sums are small against their terms
#pragma unroll
    for (int j = 0; j < NDT; ++j) { acc[j][0] = 0.0; acc[j][1] = 0.0; acc[j][2] = 0.0; acc[j][3] = 0.0; }
    double loss = 0.0;
    const int l16 = tid & 15, grp = tid >> 4;

    const int t_lo = blockIdx.x * a.g.tiles_per_wg;
    const int t_hi = t_lo + a.g.tiles_per_wg < a.g.tiles ? t_lo + a.g.tiles_per_wg : a.g.tiles;
    for (int t = t_lo; t < t_hi; ++t) {
        const int64_t row0 = (int64_t)t * PROBE_TR;
        __syncthreads();                                         // the previous tile's sums have read X' and r
        probe_stage_x(sX, a, row0);
        __syncthreads();                                         // (the first one publishes W' too)
        probe_logits(sW, sX, a, [&](int i, int c, const float (&l)[4]) {
            *reinterpret_cast<float4*>(&sR[i * LDR + c]) = make_float4(l[0], l[1], l[2], l[3]);
        });
        __syncthreads();
        for (int i = grp; i < PROBE_TR; i += 16) {               // 16 lanes per row; nothing below diverges inside a wave but the flag
            float* lr = sR + i * LDR;
            const int64_t row = row0 + i;
            int y = 0;
            bool ok = false;
            if (row < a.n) {
                y = a.classes[row];
                ok = y >= 0 && y < C;
                if (!ok && l16 == 0) atomicOr(a.flag, PROBE_ERR);        // before it indexes anything
            }
            const float ly = lr[ok ? y : 0];
            float m = -INFINITY;
            for (int c = l16; c < C; c += 16) m = fmaxf(m, lr[c]);
            m = row_max16(m);
            float s = 0.f;
            for (int c = l16; c < C; c += 16) {
                const float e = expf(lr[c] - m);
                lr[c] = e;                                       // (this lane reads it back below)
                s += e;
            }
            s = row_sum16(s);
            for (int c = l16; c < C4; c += 16) {
                float r = 0.f;
                if (ok && c < C) r = lr[c] / s - (c == y ? 1.f : 0.f);
                lr[c] = r;                                       // a refused row, a row >= n and the columns C .. C4 add nothing
            }
            if (ok && l16 == 0) loss += (double)(logf(s) + m - ly);
        }
        __syncthreads();
        if (owner) {
            for (int i = 0; i < PROBE_TR; ++i) {
                const float4 rf = *reinterpret_cast<const float4*>(&sR[i * LDR + c0]);
                const double rv[4] = {(double)rf.x, (double)rf.y, (double)rf.z, (double)rf.w};
#pragma unroll
                for (int j = 0; j < NDT; j += 4) {
                    if (j < ND && d0 + j < Dp) {
                        const float4 xv = *reinterpret_cast<const float4*>(&sX[i * Dp + d0 + j]);
                        probe_fma4d(acc[j + 0], xv.x, rv); probe_fma4d(acc[j + 1], xv.y, rv);
                        probe_fma4d(acc[j + 2], xv.z, rv); probe_fma4d(acc[j + 3], xv.w, rv);
                    }
                }
            }
        }
    }
    double* P = a.part + (int64_t)blockIdx.x * (a.D + 1) * C;
    if (owner) {
#pragma unroll
        for (int j = 0; j < NDT; ++j) {
            const int d = d0 + j;
            if (j < ND && d <= a.D) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (c0 + q < C) P[d * C + c0 + q] = acc[j][q];
            }
        }
    }
    if (l16 == 0) red[grp] = loss;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += red[k];
        a.lossp[blockIdx.x] = s;
    }
}

// out[1 + col] = (1 / n) sum over the workgroups of part[.][col] for 16 columns per block; the last block: out[0] from lossp
__global__ __launch_bounds__(256) void probe_finalize_kernel(const double* __restrict__ part, const double* __restrict__ lossp, int nwg, int ncol, int64_t n,
                                                             double* __restrict__ out) {
    __shared__ double red[16][17];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {
        double s = 0.0;
        for (int r = tid; r < nwg; r += 256) s += lossp[r];
        (&red[0][0])[tid] = s;                                   // 256 <= 16 * 17
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int k = 0; k < 256; ++k) t += (&red[0][0])[k];
            out[0] = t / (double)n;
        }
        return;
    }
    const int col = blockIdx.x * 16 + (tid & 15), rg = tid >> 4;
    double s = 0.0;
    if (col < ncol) {
#pragma unroll 8
        for (int r = rg; r < nwg; r += 16) s += part[(int64_t)r * ncol + col];
    }
    red[rg][tid & 15] = s;
    __syncthreads();
    if (tid < 16 && col < ncol) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[g][tid];
        out[1 + col] = t / (double)n;
    }
}

__global__ __launch_bounds__(256) void probe_scores_kernel(ProbeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float probe_smem[];
    float* sW = probe_smem;
    float* sX = sW + a.g.w_floats;
    probe_stage_w(sW, a);
    const int t_lo = blockIdx.x * a.g.tiles_per_wg;
    const int t_hi = t_lo + a.g.tiles_per_wg < a.g.tiles ? t_lo + a.g.tiles_per_wg : a.g.tiles;
    for (int t = t_lo; t < t_hi; ++t) {
        const int64_t row0 = (int64_t)t * PROBE_TR;
        __syncthreads();
        probe_stage_x(sX, a, row0);
        __syncthreads();
        probe_logits(sW, sX, a, [&](int i, int c, const float (&l)[4]) {
            const int64_t row = row0 + i;
            if (row < a.n) {
                float* o = a.scores + row * a.lds;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (c + q < a.C) o[c + q] = l[q];
            }
        });
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define PROBE_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

static int probe_shape_check(int64_t n, int D, int C, const char* who) {
    PROBE_REQUIRE(n >= 1 && n <= PROBE_MAX_N, "%s: n=%lld rows (1 .. %lld)", who, (long long)n, (long long)PROBE_MAX_N);
    PROBE_REQUIRE(D >= 1 && D <= PROBE_MAX_D, "%s: D=%d (1 .. %d)", who, D, PROBE_MAX_D);
    PROBE_REQUIRE(C >= 2 && C <= PROBE_MAX_C, "%s: C=%d (2 .. %d)", who, C, PROBE_MAX_C);
    PROBE_REQUIRE(D * C <= PROBE_MAX_DC, "%s: D*C=%d (at most %d: W sits in LDS)", who, D * C, PROBE_MAX_DC);
    return 0;
}

// the tile sizes, the thread ownership and the slabs: host arithmetic on (n, D, C) alone
static ProbeGeom probe_geom(int64_t n, int D, int C, bool with_r) {
    ProbeGeom g;
    g.C4 = (C + 3) & ~3;
    g.Dp = (D + 1 + 3) & ~3;
    g.LDR = g.C4 + 4;
    g.G = 256 / (g.C4 / 4);
    g.ND = ((g.Dp + g.G - 1) / g.G + 3) & ~3;
    g.tiles = (int)((n + PROBE_TR - 1) / PROBE_TR);
    // as many workgroups as keep the partials near 16 MiB, 256 .. 1024 of them
    int64_t cap = ((int64_t)16 << 20) / ((int64_t)(D + 1) * C * 8);
    cap = cap < 256 ? 256 : cap > PROBE_MAX_WG ? PROBE_MAX_WG : cap;
    g.tiles_per_wg = (int)((g.tiles + cap - 1) / cap);
    g.nwg = (g.tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;
    g.w_floats = (size_t)(D + 1) * g.C4;
    g.lds_bytes = (g.w_floats + (size_t)PROBE_TR * g.Dp + (with_r ? (size_t)PROBE_TR * g.LDR : 0)) * sizeof(float);
    return g;
}

static int64_t probe_part_bytes(const ProbeGeom& g, int D, int C) { return (int64_t)g.nwg * (D + 1) * C * 8; }

int64_t probe_xent_ws_bytes(int64_t n, int D, int C) {
    if (int rc = probe_shape_check(n, D, C, "dmvae_softmax_xent_ws_bytes")) return rc;
    const ProbeGeom g = probe_geom(n, D, C, true);
    return (probe_part_bytes(g, D, C) + (int64_t)g.nwg * 8 + 255) & ~(int64_t)255;
}

constexpr int PROBE_LDS_MAX = 156 * 1024;

template <int NDT>
static void probe_xent_dispatch(hipStream_t s, const ProbeArgs& a) {
    static bool set = false;
    if (!set) {
        (void)hipFuncSetAttribute((const void*)probe_xent_kernel<NDT>, hipFuncAttributeMaxDynamicSharedMemorySize, PROBE_LDS_MAX);
        set = true;
    }
    DMVAE_LAUNCH(probe_xent_kernel<NDT>, dim3(a.g.nwg), dim3(256), a.g.lds_bytes, s, a);
}

int probe_xent_launch(hipStream_t s, const float* Z, int64_t ldz, int64_t n, int D, const float* shift, const float* scale, const int32_t* classes, int C,
                      const float* W, int64_t ldw, const float* b, void* ws, int64_t ws_bytes, double* out, int32_t* flag) {
    const char* who = "dmvae_softmax_xent";
    if (int rc = probe_shape_check(n, D, C, who)) return rc;
    PROBE_REQUIRE(Z && classes && W && b && out && flag, "%s: null Z / classes / W / b / out / flag", who);
    PROBE_REQUIRE((shift == nullptr) == (scale == nullptr), "%s: shift and scale come together or not at all", who);
    PROBE_REQUIRE(ldz >= D && ldw >= C, "%s: ldz=%lld, ldw=%lld (ldz >= D=%d, ldw >= C=%d)", who, (long long)ldz, (long long)ldw, D, C);
    const int64_t need = probe_xent_ws_bytes(n, D, C);
    PROBE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "%s: the workspace needs %lld bytes (dmvae_softmax_xent_ws_bytes), 8-byte aligned; got %lld at %p",
                  who, (long long)need, (long long)ws_bytes, ws);
    PROBE_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
    const ProbeGeom g = probe_geom(n, D, C, true);
    PROBE_REQUIRE(g.ND <= 20 && g.lds_bytes <= (size_t)PROBE_LDS_MAX, "%s: D=%d, C=%d needs a strip of %d columns and %zu bytes of LDS", who, D, C, g.ND, g.lds_bytes);
    ProbeArgs a{Z, ldz, n, D, C, shift, scale, classes, W, ldw, b, g, (double*)ws, (double*)((char*)ws + probe_part_bytes(g, D, C)), flag, nullptr, 0};
    const int ncol = (D + 1) * C;
    ProfScope ps(s, "softmax_xent", 4.0 * (double)n * D * C, 4.0 * (double)n * (D + 1) + 8.0 * (double)g.nwg * ncol);
    if (g.ND <= 4) probe_xent_dispatch<4>(s, a);
    else if (g.ND <= 8) probe_xent_dispatch<8>(s, a);
    else if (g.ND <= 12) probe_xent_dispatch<12>(s, a);
    else probe_xent_dispatch<20>(s, a);
    DMVAE_LAUNCH(probe_finalize_kernel, dim3((ncol + 15) / 16 + 1), dim3(256), 0, s, (const double*)a.part, (const double*)a.lossp, g.nwg, ncol, n, out);
    return check_launch(who);
}

int probe_scores_launch(hipStream_t s, const float* Z, int64_t ldz, int M, int D, const float* shift, const float* scale, const float* W, int64_t ldw,
                        const float* b, int C, float* scores, int64_t lds) {
    const char* who = "dmvae_linear_scores";
    if (int rc = probe_shape_check(M, D, C, who)) return rc;
    PROBE_REQUIRE(Z && W && b && scores, "%s: null Z / W / b / scores", who);
    PROBE_REQUIRE((shift == nullptr) == (scale == nullptr), "%s: shift and scale come together or not at all", who);
    PROBE_REQUIRE(ldz >= D && ldw >= C && lds >= C, "%s: ldz=%lld, ldw=%lld, lds=%lld (ldz >= D=%d, ldw >= C=%d, lds >= C)", who, (long long)ldz, (long long)ldw,
                  (long long)lds, D, C);
    const ProbeGeom g = probe_geom(M, D, C, false);
    PROBE_REQUIRE(g.lds_bytes <= (size_t)PROBE_LDS_MAX, "%s: D=%d, C=%d needs %zu bytes of LDS", who, D, C, g.lds_bytes);
    static bool set = false;
    if (!set) {
        (void)hipFuncSetAttribute((const void*)probe_scores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PROBE_LDS_MAX);
        set = true;
    }
    ProbeArgs a{Z, ldz, (int64_t)M, D, C, shift, scale, nullptr, W, ldw, b, g, nullptr, nullptr, nullptr, scores, lds};
    ProfScope ps(s, "linear_scores", 2.0 * (double)M * D * C, 4.0 * (double)M * (D + C));
    DMVAE_LAUNCH(probe_scores_kernel, dim3(g.nwg), dim3(256), g.lds_bytes, s, a);
    return check_launch(who);
}

}  // namespace dmvae
