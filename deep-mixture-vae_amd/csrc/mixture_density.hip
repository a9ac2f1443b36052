// The log-density of points under a diagonal Gaussian mixture with any number of components, on the device:
//   out[i] = logsumexp_j ( log_w[j] - 1/2 sum_d ((z_id - mu_jd)^2 exp(-lv_jd) + lv_jd) ) - (D/2) log 2 pi        i < M, j < J
// With the N encoder posteriors as components this is log q(z), the aggregate posterior at a point; with the K prior rows log p(z).
// An all-pairs computation, M x J x D, that stores no M x J array:
//   md_prepare_kernel   one thread per component: iv[j][d] = __expf(-lv) and c_j = log_w[j] - 1/2 sum_d lv (the sum in double) into the workspace
//   md_pad_kernel       the points into the workspace as [ceil16(M)][ceil4(D)], zeros in the padding: the pair kernel reads them without a bound
//   md_pairs_kernel     a 256-thread workgroup owns 16 points and a stretch of 256-component tiles; a thread owns ONE component per tile.  mu and iv pass
//                       through LDS 16 columns of D at a time (row stride 20 floats: the 16-byte reads of 16 lanes fall into 64 distinct banks), the
//                       16 points are uniform over the workgroup and come by scalar loads (s_load_dwordx4 of the padded copy; an LDS tile of them read
//                       as broadcasts cost 16 of the 18 LDS reads per four columns).  The quadratic form is taken in the DIFFERENCE form -- e = z - mu, e * e, fma with iv -- d ascending:
//                       the norm expansion cancels at posterior variances of 1e-6.  A thread keeps the 16 forms of its component across the chunks, then
//                       t = c_j - Q / 2 goes into a running (max f32, scaled sum f64) per point: one __expf per pair, the sum in double, so that the
//                       number of tiles a thread walks does not enter the error.  At the end the 256 pairs of a point are joined in a fixed order (xor
//                       butterfly, then the four waves in order).  A component of weight 0 (c_j = -inf) and the masked tail of the last tile never
//                       enter a pair; a point whose pairs are all empty gets -inf.  No NaN is formed from finite inputs.
//   md_join_kernel      few points, many components: J is split across blockIdx.y into partial pairs [nsplit][M] (every one written before it is
//                       read), joined here in ascending order.  The split is a function of (M, J, D) alone.
// and, for the posterior diagnostics:
//   md_sample_kernel    z = mu + exp(lv / 2) eps and a = log q(z | x) = -1/2 sum_d (eps^2 + lv) - (D/2) log 2 pi, 16 lanes per row, formed in double
//   md_colsum_kernel /  column mean of mu, its population variance TWO-PASS (centred on the mean of the first pass) and the column mean of exp(lv),
//   md_colfin_kernel    all in double: a thread adds every 16th row of its row block in ascending order, the 16 row groups and then the row blocks are
//                       added in ascending order
//   md_sum_kernel       sum of an f32 vector in double: a thread adds a contiguous stretch in order, thread 0 the 256 stretches
// No float atomics, no spinning, every loop bounded by the arguments: two calls on the same inputs return the same bits.
#include <math.h>

#include "mixture_density.h"
#include "lse.h"                                 // MdLse, md_join: the running logsumexp pair

namespace dmvae {

constexpr int MD_PTS = 16, MD_COLS = 256, MD_DC = 16;
constexpr int MD_LD = MD_DC + 4;                 // row stride of the component tiles in LDS
constexpr int MD_TARGET_WGS = 1024;              // fewer point groups than this: J is split until the grid has about as many workgroups
constexpr int MD_STAT_BLOCKS = 128;              // row blocks of the column statistics, at most
constexpr double MD_HALF_LOG_2PI = 0.91893853320467274178;

struct MdWs {
    float* iv;      // [J][D] exp(-lv)
    float* cj;      // [J] log_w - 1/2 sum_d lv
    float* zp;      // [ceil16(M)][ceil4(D)] the points, zero-padded
    float* pm;      // [nsplit][M] partial maxima
    double* ps;     // [nsplit][M] partial scaled sums
};

__global__ __launch_bounds__(256) void md_prepare_kernel(const float* __restrict__ log_var, int64_t ldv, const float* __restrict__ log_w, int J, int D,
                                                         float* __restrict__ iv, float* __restrict__ cj) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= J) return;
    const float* lv = log_var + (int64_t)j * ldv;
    float* o = iv + (int64_t)j * D;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const float l = lv[d];
        o[d] = __expf(-l);
        s += (double)l;
    }
    cj[j] = (float)((log_w ? (double)log_w[j] : 0.0) - 0.5 * s);
}

// the points as the pair kernel reads them: every row group whole, every row a multiple of four columns, zeros in the padding
__global__ __launch_bounds__(256) void md_pad_kernel(const float* __restrict__ Z, int64_t ldz, int M, int D, int Mp, int Dp, float* __restrict__ zp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Mp * Dp) return;
    const int i = (int)(idx / Dp), d = (int)(idx % Dp);
    zp[idx] = (i < M && d < D) ? Z[(int64_t)i * ldz + d] : 0.f;
}

__device__ __forceinline__ float md_finish(MdLse v, double add) {
    return v.s > 0.0 ? (float)((double)v.m + log(v.s) + add) : -INFINITY;
}

struct MdArgs {
    const float* zp; int ldzp; int M, D;          // the points, zero-padded to [ceil16(M)][ceil4(D)] by md_prepare_kernel
    const float* mean; int64_t ldm; const float* iv; const float* cj; int J;
    int tiles, tiles_per_split, nsplit;
    double add;                                  // -(D/2) log 2 pi, and -log J under uniform weights
    float* out; float* pm; double* ps;
};

__global__ __launch_bounds__(256) void md_pairs_kernel(MdArgs a) {
    __shared__ __attribute__((aligned(16))) float mu[MD_COLS][MD_LD];
    __shared__ __attribute__((aligned(16))) float sv[MD_COLS][MD_LD];
    __shared__ float redm[4][MD_PTS];
    __shared__ double reds[4][MD_PTS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i0 = blockIdx.x * MD_PTS, split = blockIdx.y;
    const int M = a.M, D = a.D, J = a.J;
    const int nchunk = (D + MD_DC - 1) / MD_DC;
    const int t_lo = split * a.tiles_per_split;
    const int t_hi = t_lo + a.tiles_per_split < a.tiles ? t_lo + a.tiles_per_split : a.tiles;

    float m[MD_PTS];
    double s[MD_PTS];
#pragma unroll
    for (int r = 0; r < MD_PTS; ++r) { m[r] = -INFINITY; s[r] = 0.0; }
    const float* __restrict__ zrow = a.zp + (int64_t)i0 * a.ldzp;   // uniform over the workgroup: the points are read by scalar loads

    for (int t = t_lo; t < t_hi; ++t) {
        const int j = t * MD_COLS + tid;                         // < 2^20 + 256
        const float c = j < J ? a.cj[j] : -INFINITY;             // the last tile is ragged
        float acc[MD_PTS];
#pragma unroll
        for (int r = 0; r < MD_PTS; ++r) acc[r] = 0.f;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int d0 = ch * MD_DC;
            const int dn = D - d0 < MD_DC ? D - d0 : MD_DC;
            const int dn4 = (dn + 3) & ~3;                       // columns dn .. dn4 are staged as zeros on every side: (0 - 0)^2 * 0
            __syncthreads();                                     // the previous chunk's reads are done
            for (int idx = tid; idx < MD_COLS * MD_DC; idx += 256) {
                const int r = idx >> 4, cc = idx & 15;
                if (cc < dn4) {
                    const int jj = t * MD_COLS + r;
                    const bool ok = jj < J && cc < dn;
                    mu[r][cc] = ok ? a.mean[(int64_t)jj * a.ldm + d0 + cc] : 0.f;
                    sv[r][cc] = ok ? a.iv[(int64_t)jj * D + d0 + cc] : 0.f;
                }
            }
            __syncthreads();
            for (int d = 0; d < dn4; d += 4) {
                const float4 v = *reinterpret_cast<const float4*>(&mu[tid][d]);
                const float4 q = *reinterpret_cast<const float4*>(&sv[tid][d]);
#pragma unroll
                for (int r = 0; r < MD_PTS; ++r) {
                    const float4 u = *reinterpret_cast<const float4*>(zrow + r * a.ldzp + d0 + d);
                    const float e0 = u.x - v.x, e1 = u.y - v.y, e2 = u.z - v.z, e3 = u.w - v.w;
                    acc[r] = fmaf(e0 * e0, q.x, acc[r]);
                    acc[r] = fmaf(e1 * e1, q.y, acc[r]);
                    acc[r] = fmaf(e2 * e2, q.z, acc[r]);
                    acc[r] = fmaf(e3 * e3, q.w, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < MD_PTS; ++r) {
            const float x = fmaf(-0.5f, acc[r], c);              // -inf for a weight of 0 and for the masked tail; a NaN (inf * 0) fails both tests below
            const float e = __expf(-fabsf(x - m[r]));            // (unused where x = m = -inf makes it a NaN)
            if (x > m[r]) { s[r] = s[r] * (double)e + 1.0; m[r] = x; }
            else if (x > -INFINITY) s[r] += (double)e;
        }
    }

    // the 256 pairs of every point, in a fixed order
#pragma unroll
    for (int r = 0; r < MD_PTS; ++r) {
        MdLse v{m[r], s[r]};
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = md_join(v, MdLse{__shfl_xor(v.m, o, 64), __shfl_xor(v.s, o, 64)});
        if (lane == 0) { redm[w][r] = v.m; reds[w][r] = v.s; }
    }
    __syncthreads();
    if (tid < MD_PTS && i0 + tid < M) {
        MdLse v{redm[0][tid], reds[0][tid]};
#pragma unroll
        for (int k = 1; k < 4; ++k) v = md_join(v, MdLse{redm[k][tid], reds[k][tid]});
        if (a.nsplit == 1) a.out[i0 + tid] = md_finish(v, a.add);
        else {
            a.pm[(int64_t)split * M + i0 + tid] = v.m;
            a.ps[(int64_t)split * M + i0 + tid] = v.s;
        }
    }
}

__global__ __launch_bounds__(256) void md_join_kernel(const float* __restrict__ pm, const double* __restrict__ ps, int M, int nsplit, double add,
                                                      float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    MdLse v{pm[i], ps[i]};
    for (int k = 1; k < nsplit; ++k) v = md_join(v, MdLse{pm[(int64_t)k * M + i], ps[(int64_t)k * M + i]});
    out[i] = md_finish(v, add);
}

// ------------------------------------------------------------------------------------------------------- samples of the posteriors
__global__ __launch_bounds__(256) void md_sample_kernel(const float* __restrict__ mean, int64_t ldm, const float* __restrict__ log_var, int64_t ldv, int n, int D,
                                                        const float* __restrict__ eps, int64_t ld_eps, uint64_t seed, uint64_t counter, int64_t pos0,
                                                        float* __restrict__ Z, int64_t ldz, float* __restrict__ logq) {
    const int lane = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = i < n;
    double acc = 0.0;
    if (valid) {
        for (int d = lane; d < D; d += 16) {
            const double l = (double)log_var[i * ldv + d];
            const double e = (double)(eps ? eps[i * ld_eps + d] : philox_normal_at(seed, counter, MD_PHILOX_STREAM, (uint64_t)(pos0 + i) * (uint64_t)D + (uint64_t)d));
            Z[i * ldz + d] = (float)((double)mean[i * ldm + d] + exp(0.5 * l) * e);
            acc += e * e + l;
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
    if (valid && lane == 0) logq[i] = (float)(-0.5 * acc - (double)D * MD_HALF_LOG_2PI);
}

// ------------------------------------------------------------------------------------------------------- column statistics
// pass 0: sums of mu and of exp(lv); pass 1: sums of (mu - out[0][col])^2.  part [2][nblk][D]
__global__ __launch_bounds__(256) void md_colsum_kernel(const float* __restrict__ mean, int64_t ldm, const float* __restrict__ log_var, int64_t ldv, int n, int D,
                                                        int rows_per_block, int pass, const double* __restrict__ out, double* __restrict__ part) {
    __shared__ double red[2][16][17];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + cl, nblk = gridDim.y;
    const int lo = blockIdx.y * rows_per_block;
    const int hi = lo + rows_per_block < n ? lo + rows_per_block : n;
    double s0 = 0.0, s1 = 0.0;
    if (col < D) {
        if (pass == 0) {
            for (int r = lo + rg; r < hi; r += 16) {
                s0 += (double)mean[(int64_t)r * ldm + col];
                s1 += exp((double)log_var[(int64_t)r * ldv + col]);
            }
        } else {
            const double mu = out[col];
            for (int r = lo + rg; r < hi; r += 16) {
                const double e = (double)mean[(int64_t)r * ldm + col] - mu;
                s0 += e * e;
            }
        }
    }
    red[0][rg][cl] = s0;
    red[1][rg][cl] = s1;
    __syncthreads();
    if (rg == 0 && col < D) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) { t0 += red[0][g][cl]; t1 += red[1][g][cl]; }
        part[(int64_t)blockIdx.y * D + col] = t0;
        if (pass == 0) part[((int64_t)nblk + blockIdx.y) * D + col] = t1;
    }
}

__global__ __launch_bounds__(256) void md_colfin_kernel(const double* __restrict__ part, int nblk, int n, int D, int pass, double* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= D) return;
    double t0 = 0.0, t1 = 0.0;
    for (int b = 0; b < nblk; ++b) {
        t0 += part[(int64_t)b * D + col];
        if (pass == 0) t1 += part[((int64_t)nblk + b) * D + col];
    }
    if (pass == 0) {
        out[col] = t0 / (double)n;
        out[2 * (int64_t)D + col] = t1 / (double)n;
    } else {
        out[(int64_t)D + col] = t0 / (double)n;
    }
}

__global__ __launch_bounds__(256) void md_sum_kernel(const float* __restrict__ in, int64_t n, double* __restrict__ out) {
    __shared__ double part[256];
    const int64_t chunk = (n + 255) / 256, b = threadIdx.x * chunk;
    double s = 0.0;
    for (int64_t k = b; k < b + chunk && k < n; ++k) s += (double)in[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += part[k];
        out[0] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int64_t md_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
static int64_t md_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
static int64_t md_up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

MdSplit mixture_logpdf_split(int M, int J, int D) {
    (void)D;                                                     // the split does not depend on D today; the signature is the contract
    MdSplit sp;
    sp.tiles = (J + MD_COLS - 1) / MD_COLS;
    const int groups = (M + MD_PTS - 1) / MD_PTS;
    int want = (MD_TARGET_WGS + groups - 1) / groups;            // 1 from MD_TARGET_WGS point groups on: M > 16 (MD_TARGET_WGS - 1)
    if (want > sp.tiles) want = sp.tiles;
    sp.tiles_per_split = (sp.tiles + want - 1) / want;
    sp.nsplit = (sp.tiles + sp.tiles_per_split - 1) / sp.tiles_per_split;      // no empty split
    return sp;
}

static int64_t md_carve(int64_t M, int64_t J, int64_t D, char* base, MdWs* w) {
    const MdSplit sp = mixture_logpdf_split((int)M, (int)J, (int)D);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += md_up256(bytes); return p; };
    MdWs t;
    t.iv = (float*)take(J * D * 4);
    t.cj = (float*)take(J * 4);
    t.zp = (float*)take(md_up16(M) * md_up4(D) * 4);
    t.pm = (float*)take((int64_t)sp.nsplit * M * 4);
    t.ps = (double*)take((int64_t)sp.nsplit * M * 8);
    if (w) *w = t;
    return off;
}

static int md_shape_check(int64_t M, int64_t J, int64_t D, const char* who) {
    DMVAE_REQUIRE(M >= 1 && M <= MD_MAX_ROWS && J >= 1 && J <= MD_MAX_ROWS, "%s: M=%lld, J=%lld (1 <= M, J <= %d)", who, (long long)M, (long long)J, MD_MAX_ROWS);
    DMVAE_REQUIRE(D >= 1 && D <= (1 << 20), "%s: D=%lld (1 <= D <= 2^20)", who, (long long)D);
    return 0;
}

int64_t mixture_logpdf_ws_bytes(int64_t M, int64_t J, int64_t D) {
    if (int rc = md_shape_check(M, J, D, "dmvae_mixture_logpdf_ws_bytes")) return rc;
    return md_carve(M, J, D, nullptr, nullptr);
}

int mixture_logpdf_launch(hipStream_t s, const float* Z, int64_t ldz, int M, int D, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int J,
                          const float* log_w, void* ws, int64_t ws_bytes, float* out) {
    const char* who = "dmvae_mixture_logpdf";
    if (int rc = md_shape_check(M, J, D, who)) return rc;
    DMVAE_REQUIRE(Z && mean && log_var && out, "%s: Z, mean, log_var and out must be given", who);
    DMVAE_REQUIRE(ldz >= D && ldm >= D && ldv >= D, "%s: D=%d, ldz=%lld, ldm=%lld, ldv=%lld (every ld >= D)", who, D, (long long)ldz, (long long)ldm, (long long)ldv);
    const int64_t need = md_carve(M, J, D, nullptr, nullptr);
    DMVAE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "%s: the workspace needs %lld bytes (dmvae_mixture_logpdf_ws_bytes), 8-byte aligned; got %lld at %p",
                  who, (long long)need, (long long)ws_bytes, ws);
    MdWs w;
    md_carve(M, J, D, (char*)ws, &w);
    const MdSplit sp = mixture_logpdf_split(M, J, D);
    const int groups = (M + MD_PTS - 1) / MD_PTS;
    ProfScope ps(s, "mixture_logpdf", (double)M * J * (3.0 * D + 6.0), 8.0 * J * D * ((double)groups + 1.0) + 4.0 * M * D * sp.nsplit);
    DMVAE_LAUNCH(md_prepare_kernel, dim3((J + 255) / 256), dim3(256), 0, s, log_var, ldv, log_w, J, D, w.iv, w.cj);
    const double add = -(double)D * MD_HALF_LOG_2PI - (log_w ? 0.0 : log((double)J));
    const int Mp = (int)md_up16(M), Dp = (int)md_up4(D);
    DMVAE_LAUNCH(md_pad_kernel, dim3((unsigned)(((int64_t)Mp * Dp + 255) / 256)), dim3(256), 0, s, Z, ldz, M, D, Mp, Dp, w.zp);
    const MdArgs a{w.zp, Dp, M, D, mean, ldm, w.iv, w.cj, J, sp.tiles, sp.tiles_per_split, sp.nsplit, add, out, w.pm, w.ps};
    DMVAE_LAUNCH(md_pairs_kernel, dim3(groups, sp.nsplit), dim3(256), 0, s, a);
    if (sp.nsplit > 1) DMVAE_LAUNCH(md_join_kernel, dim3((M + 255) / 256), dim3(256), 0, s, w.pm, w.ps, M, sp.nsplit, add, out);
    return check_launch(who);
}

int posterior_sample_launch(hipStream_t s, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, const float* eps, int64_t ld_eps,
                            uint64_t seed, uint64_t counter, int64_t pos0, float* Z, int64_t ldz, float* logq) {
    const char* who = "dmvae_posterior_sample";
    DMVAE_REQUIRE(n >= 1 && n <= MD_MAX_ROWS && D >= 1 && D <= (1 << 20), "%s: n=%d, D=%d (1 <= n, D <= 2^20)", who, n, D);
    DMVAE_REQUIRE(mean && log_var && Z && logq, "%s: mean, log_var, Z and logq must be given", who);
    DMVAE_REQUIRE(ldm >= D && ldv >= D && ldz >= D && (!eps || ld_eps >= D), "%s: D=%d, ldm=%lld, ldv=%lld, ldz=%lld, ld_eps=%lld (every ld >= D)", who, D,
                  (long long)ldm, (long long)ldv, (long long)ldz, (long long)ld_eps);
    DMVAE_REQUIRE(pos0 >= 0 && pos0 <= ((int64_t)1 << 34), "%s: pos0=%lld (0 <= pos0 <= 2^34: the Philox block index stays below 2^56)", who, (long long)pos0);
    ProfScope ps(s, "posterior_sample", 8.0 * n * D, 4.0 * n * D * (eps ? 4.0 : 3.0));
    DMVAE_LAUNCH(md_sample_kernel, dim3((n + 15) / 16), dim3(256), 0, s, mean, ldm, log_var, ldv, n, D, eps, ld_eps, seed, counter, pos0, Z, ldz, logq);
    return check_launch(who);
}

static void md_stat_blocks(int64_t n, int* rows_per_block, int* nblk) {
    int64_t per = (n + MD_STAT_BLOCKS - 1) / MD_STAT_BLOCKS;
    per = (per + 15) / 16 * 16;
    *rows_per_block = (int)per;
    *nblk = (int)((n + per - 1) / per);
}

static int md_stat_check(int64_t n, int64_t D, const char* who) {
    DMVAE_REQUIRE(n >= 1 && n <= MD_MAX_ROWS && D >= 1 && D <= (1 << 20), "%s: n=%lld, D=%lld (1 <= n, D <= 2^20)", who, (long long)n, (long long)D);
    return 0;
}

int64_t column_stats_ws_bytes(int64_t n, int64_t D) {
    if (int rc = md_stat_check(n, D, "dmvae_column_stats_ws_bytes")) return rc;
    int per, nblk;
    md_stat_blocks(n, &per, &nblk);
    return md_up256(2 * (int64_t)nblk * D * 8);
}

int column_stats_launch(hipStream_t s, const float* mean, int64_t ldm, const float* log_var, int64_t ldv, int n, int D, void* ws, int64_t ws_bytes, double* out) {
    const char* who = "dmvae_column_stats";
    if (int rc = md_stat_check(n, D, who)) return rc;
    DMVAE_REQUIRE(mean && log_var && out && ((uintptr_t)out & 7) == 0, "%s: mean, log_var and out (8-byte aligned) must be given", who);
    DMVAE_REQUIRE(ldm >= D && ldv >= D, "%s: D=%d, ldm=%lld, ldv=%lld (every ld >= D)", who, D, (long long)ldm, (long long)ldv);
    const int64_t need = column_stats_ws_bytes(n, D);
    DMVAE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "%s: the workspace needs %lld bytes (dmvae_column_stats_ws_bytes), 8-byte aligned; got %lld at %p",
                  who, (long long)need, (long long)ws_bytes, ws);
    int per, nblk;
    md_stat_blocks(n, &per, &nblk);
    double* part = (double*)ws;
    ProfScope ps(s, "column_stats", 6.0 * n * D, 12.0 * n * D);
    for (int pass = 0; pass < 2; ++pass) {
        DMVAE_LAUNCH(md_colsum_kernel, dim3((D + 15) / 16, nblk), dim3(256), 0, s, mean, ldm, log_var, ldv, n, D, per, pass, (const double*)out, part);
        DMVAE_LAUNCH(md_colfin_kernel, dim3((D + 255) / 256), dim3(256), 0, s, (const double*)part, nblk, n, D, pass, out);
    }
    return check_launch(who);
}

int sum_f64_launch(hipStream_t s, const float* x, int64_t n, double* out) {
    const char* who = "dmvae_sum_f64";
    DMVAE_REQUIRE(x && out && ((uintptr_t)out & 7) == 0, "%s: x and out (8-byte aligned) must be given", who);
    DMVAE_REQUIRE(n >= 1 && n <= ((int64_t)1 << 31), "%s: n=%lld (1 <= n <= 2^31)", who, (long long)n);
    DMVAE_LAUNCH(md_sum_kernel, dim3(1), dim3(256), 0, s, x, n, out);
    return check_launch(who);
}

}  // namespace dmvae
