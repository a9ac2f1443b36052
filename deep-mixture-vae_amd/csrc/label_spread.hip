// Label spreading over a symmetric sparse graph (Zhou et al. 2004, "Learning with local and global consistency"): the few-label evaluator's hot
// path.  W is CSR (indptr int64 [N + 1], indices int32 ascending within a row, values f32), symmetric, without a diagonal -- what
// dmvae_hip.tsne.knn_symmetrize builds from the lists of dmvae_knn.
//
//   graph_sym_normalize   d_i = sum_j W_ij in float64 in CSR order, r_i = d_i^-1/2 rounded once to f32 (0 for a row without edges),
//                         S_ij = (W_ij r_i) r_j in f32.  Two launches: the degrees (a thread per row: the order of the sum is the row's), then
//                         the entries (8 lanes per row).  A column outside [0, N) sets SPREAD_ERR_INDEX, adds nothing to d and gets S = 0.
//   label_spread          n_iter launches of spread_iter_kernel, F' = alpha S F + (1 - alpha) Y, per element
//                           acc = fmaf(S_ij, F[j][c], acc) over the row's entries ascending from 0;   F'[i][c] = fmaf(alpha, acc, (1 - alpha) [y_i == c])
//                         The kernel boundary is the only ordering between workgroups: a launch reads what the previous one stored with plain
//                         loads, no fence, no scope bit, nothing spins.
//
// Layout of an iteration.  The work is gathers of short rows: C columns padded to Cp = 4 nch floats in the workspace copies of F, so a neighbour's
// row is nch 16-byte loads.  G = the power of two >= nch (at most 64) lanes share a row, a chunk each, so a wave holds 64 / G rows (C = 10: 3
// chunks, 4 lanes, 16 rows); past 256 columns the 64 lanes take a further pass over the row's entries per 64 chunks.  Every lane of a row's group
// walks the row's entries in the same ascending order and owns its columns' chains: an element's bits do not depend on the launch shape.  Entries
// are taken 8 at a time -- the next 8 (column, S) pairs are requested before the 8 neighbour rows of the current ones, so a long row streams
// instead of paying one round trip per entry -- and the four waves of a workgroup never meet at a barrier behind their rows: a hub row of
// degree in the hundreds delays the 64 / G rows of its own wave and nobody else.
// change_t = max |F' - F| over the C columns: every wave leaves the maximum of its rows as the bits of a non-negative float (unsigned order = float
// order, a NaN above everything) in a slot of its own; workgroup 0 of the NEXT launch joins the slots into change[t] before its own rows, a
// one-workgroup launch joins the last.  No atomics on floats, no order: two runs give the same bits.
// F ping-pongs between two padded workspace buffers; the last launch writes the caller's [N][ldf], columns < C only.  The first launch reads
// F_in with scalar loads where its stride or address does not allow 16-byte ones; F_in = NULL reads zeros through the same fmaf chain.
#include <math.h>

#include "label_spread.h"

namespace dmvae {

constexpr int SPREAD_BATCH = 8;              // entries of a row in flight

struct SpreadArgs {
    const int64_t* indptr; const int32_t* indices; const float* s; const int32_t* labels;
    const float* fin; int64_t ldin; int vin;          // null: zeros; vin: rows are read in 16-byte chunks (ldin >= Cp, aligned)
    float* fout; int64_t ldout; int vout;             // vout: a workspace buffer, all Cp columns in 16-byte chunks; else the caller's, columns < C
    int N, C, nch, G, gshift, npass;
    int64_t nnz;
    float alpha, beta;                                // beta = 1 - alpha, rounded once on the host
    const unsigned int* part_prev; int n_prev; float* change_prev;      // the previous launch's per-wave maxima and where their join goes (null: none)
    unsigned int* part;                               // this launch's, one per wave
    int32_t* err;
};

// how a launch reads its input F: no input (zeros), 16-byte chunks, or scalars (any stride and address).  A template argument, and every load
// below unconditional -- an absent entry reads the row's own F and is dropped by a select: with loads under per-lane conditions the compiler
// put each behind a branch and a wait of its own, one round trip per entry (measured: 190 ns per entry of a hub row).
enum { SPREAD_IN_ZERO = 0, SPREAD_IN_VEC = 1, SPREAD_IN_SCALAR = 2 };

template <int MODE>
__device__ __forceinline__ f32x4 spread_chunk(const float* row, int q, int C) {
    if constexpr (MODE == SPREAD_IN_ZERO) return f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == SPREAD_IN_VEC) return *reinterpret_cast<const f32x4*>(row + 4 * q);
    const int c = 4 * q, last = C - 1;                             // (c <= last: q < nch)
    const float x = row[c], y = row[min(c + 1, last)], z = row[min(c + 2, last)], w = row[min(c + 3, last)];
    return f32x4{x, c + 1 < C ? y : 0.f, c + 2 < C ? z : 0.f, c + 3 < C ? w : 0.f};
}

// max over n slots by the 256 threads of a workgroup -> *out (thread 0)
__device__ __forceinline__ void spread_join(const unsigned int* part, int n, float* out) {
    __shared__ unsigned int red[SPREAD_WAVES];
    unsigned int m = 0;
    for (int i = threadIdx.x; i < n; i += 64 * SPREAD_WAVES) m = max(m, part[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < SPREAD_WAVES; ++k) m = max(m, red[k]);
        *out = __uint_as_float(m);
    }
}

__global__ __launch_bounds__(64 * SPREAD_WAVES) void spread_join_kernel(const unsigned int* part, int n, float* out) { spread_join(part, n, out); }

// (n_iter = 1 continued in place: the launch wrote a workspace buffer, this copies its C columns to the caller's rows)
__global__ __launch_bounds__(256) void spread_unpack_kernel(const float* src, int64_t lds, float* dst, int64_t ldd, int N, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * C) return;
    const int64_t r = i / C;
    const int c = (int)(i - r * C);
    dst[r * ldd + c] = src[r * lds + c];
}

template <int MODE>
__global__ __launch_bounds__(64 * SPREAD_WAVES) void spread_iter_kernel(SpreadArgs a) {
    if (blockIdx.x == 0 && a.part_prev) spread_join(a.part_prev, a.n_prev, a.change_prev);      // (workgroup-uniform: the barrier inside is safe)

    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * SPREAD_WAVES + (threadIdx.x >> 6);
    const int sub = lane & (a.G - 1);
    const int64_t row = wave * (64 >> a.gshift) + (lane >> a.gshift);
    const int N = a.N, C = a.C;
    unsigned int mx = 0;

    if (row < N) {
        int64_t beg = a.indptr[row], end = a.indptr[row + 1];
        beg = beg < 0 ? 0 : (beg > a.nnz ? a.nnz : beg);                   // nothing outside the nnz entries is read, whatever indptr holds
        end = end < beg ? beg : (end > a.nnz ? a.nnz : end);
        int y = a.labels[row];
        if (y < -1 || y >= C) {
            if (sub == 0) atomicOr(a.err, SPREAD_ERR_LABEL);
            y = -1;
        }
        const float* own = a.fin + row * a.ldin;                           // (never read in SPREAD_IN_ZERO)
        bool bad = false;
        for (int p = 0; p < a.npass; ++p) {
            const int q = sub + p * a.G;
            if (q >= a.nch) break;
            f32x4 acc{0.f, 0.f, 0.f, 0.f};
            int32_t col[SPREAD_BATCH], ncol[SPREAD_BATCH];
            float sv[SPREAD_BATCH], nsv[SPREAD_BATCH];
#pragma unroll
            for (int u = 0; u < SPREAD_BATCH; ++u) {
                const int64_t e = beg + u;
                col[u] = e < end ? a.indices[e] : -1;
                sv[u] = e < end ? a.s[e] : 0.f;
            }
            for (int64_t e0 = beg; e0 < end; e0 += SPREAD_BATCH) {
#pragma unroll
                for (int u = 0; u < SPREAD_BATCH; ++u) {                    // the next batch's pairs: in flight beside this batch's rows
                    const int64_t e = e0 + SPREAD_BATCH + u;
                    ncol[u] = e < end ? a.indices[e] : -1;
                    nsv[u] = e < end ? a.s[e] : 0.f;
                }
                f32x4 f[SPREAD_BATCH];
#pragma unroll
                for (int u = 0; u < SPREAD_BATCH; ++u) {
                    const bool ok = (unsigned int)col[u] < (unsigned int)N;
                    bad = bad || (e0 + u < end && !ok);
                    col[u] = ok ? col[u] : -1;
                    f[u] = spread_chunk<MODE>(ok ? a.fin + (int64_t)col[u] * a.ldin : own, q, C);
                }
#pragma unroll
                for (int u = 0; u < SPREAD_BATCH; ++u) {
                    const bool ok = col[u] >= 0;                            // (an absent entry leaves acc alone: fmaf(0, 0, -0) would be +0)
                    acc.x = ok ? fmaf(sv[u], f[u].x, acc.x) : acc.x; acc.y = ok ? fmaf(sv[u], f[u].y, acc.y) : acc.y;
                    acc.z = ok ? fmaf(sv[u], f[u].z, acc.z) : acc.z; acc.w = ok ? fmaf(sv[u], f[u].w, acc.w) : acc.w;
                }
#pragma unroll
                for (int u = 0; u < SPREAD_BATCH; ++u) { col[u] = ncol[u]; sv[u] = nsv[u]; }
            }
            const f32x4 old = spread_chunk<MODE>(own, q, C);
            const int c0 = 4 * q;
            f32x4 out;
            out.x = fmaf(a.alpha, acc.x, c0 == y ? a.beta : 0.f);
            out.y = fmaf(a.alpha, acc.y, c0 + 1 == y ? a.beta : 0.f);
            out.z = fmaf(a.alpha, acc.z, c0 + 2 == y ? a.beta : 0.f);
            out.w = fmaf(a.alpha, acc.w, c0 + 3 == y ? a.beta : 0.f);
            if (c0 < C) mx = max(mx, __float_as_uint(fabsf(out.x - old.x)));
            if (c0 + 1 < C) mx = max(mx, __float_as_uint(fabsf(out.y - old.y)));
            if (c0 + 2 < C) mx = max(mx, __float_as_uint(fabsf(out.z - old.z)));
            if (c0 + 3 < C) mx = max(mx, __float_as_uint(fabsf(out.w - old.w)));
            float* dst = a.fout + row * a.ldout + c0;
            if (a.vout) {
                *reinterpret_cast<f32x4*>(dst) = out;
            } else {
                if (c0 < C) dst[0] = out.x;
                if (c0 + 1 < C) dst[1] = out.y;
                if (c0 + 2 < C) dst[2] = out.z;
                if (c0 + 3 < C) dst[3] = out.w;
            }
        }
        if (bad && sub == 0) atomicOr(a.err, SPREAD_ERR_INDEX);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, o, 64));
    if (lane == 0) a.part[wave] = mx;
}

// ---------------------------------------------------------------------------------------------------------------- the normalisation
__global__ __launch_bounds__(256) void spread_degree_kernel(const int64_t* indptr, const int32_t* indices, const float* w, int N, int64_t nnz, float* r,
                                                            int32_t* err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int64_t beg = indptr[i], end = indptr[i + 1];
    beg = beg < 0 ? 0 : (beg > nnz ? nnz : beg);
    end = end < beg ? beg : (end > nnz ? nnz : end);
    double d = 0.0;
    bool bad = false;
    for (int64_t e = beg; e < end; ++e) {
        if ((unsigned int)indices[e] >= (unsigned int)N) bad = true;
        else d += (double)w[e];
    }
    r[i] = d > 0.0 ? (float)(1.0 / sqrt(d)) : 0.f;
    if (bad) atomicOr(err, SPREAD_ERR_INDEX);
}

__global__ __launch_bounds__(256) void spread_scale_kernel(const int64_t* indptr, const int32_t* indices, const float* w, int N, int64_t nnz, const float* r,
                                                           float* s) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t >> 3;
    if (i >= N) return;
    int64_t beg = indptr[i], end = indptr[i + 1];
    beg = beg < 0 ? 0 : (beg > nnz ? nnz : beg);
    end = end < beg ? beg : (end > nnz ? nnz : end);
    const float ri = r[i];
    for (int64_t e = beg + (t & 7); e < end; e += 8) {
        const int32_t j = indices[e];
        s[e] = (unsigned int)j < (unsigned int)N ? (w[e] * ri) * r[j] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define SPREAD_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

SpreadShape spread_shape(int C) {
    SpreadShape h;
    h.Cp = (C + 3) & ~3;
    h.nch = h.Cp / 4;
    h.G = 1;
    while (h.G < h.nch && h.G < 64) h.G *= 2;
    h.rows_per_wave = 64 / h.G;
    h.npass = (h.nch + h.G - 1) / h.G;
    return h;
}

int64_t spread_n_waves(int64_t N, int C) {
    const int64_t rpw = spread_shape(C).rows_per_wave;
    const int64_t nw = (N + rpw - 1) / rpw;
    return (nw + SPREAD_WAVES - 1) / SPREAD_WAVES * SPREAD_WAVES;
}

static int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the workspace: two padded copies of F [N][Cp] f32, two sets of per-wave maxima (u32), each section on a 256-byte boundary
int64_t label_spread_ws_bytes(int64_t N, int C) {
    if (N < 1 || N > SPREAD_MAX_N || C < SPREAD_MIN_C || C > SPREAD_MAX_C) {
        set_error("dmvae_label_spread_ws_bytes: N=%lld (1 .. %d), C=%d (%d .. %d)", (long long)N, SPREAD_MAX_N, C, SPREAD_MIN_C, SPREAD_MAX_C);
        return DMVAE_EINVAL;
    }
    return 2 * align256(N * spread_shape(C).Cp * 4) + 2 * align256(spread_n_waves(N, C) * 4);
}

int graph_sym_normalize_launch(hipStream_t st, const int64_t* indptr, const int32_t* indices, const float* w, int N, int64_t nnz, float* s, float* r,
                               int32_t* err_flag) {
    const char* who = "dmvae_graph_sym_normalize";
    SPREAD_REQUIRE(N >= 1 && N <= SPREAD_MAX_N, "%s: N=%d (1 .. %d)", who, N, SPREAD_MAX_N);
    SPREAD_REQUIRE(nnz >= 0, "%s: nnz=%lld (>= 0)", who, (long long)nnz);
    SPREAD_REQUIRE(indptr && r && err_flag, "%s: null indptr / r / err_flag", who);
    SPREAD_REQUIRE(nnz == 0 || (indices && w && s), "%s: null indices / w / s with nnz=%lld", who, (long long)nnz);
    ProfScope ps(st, "graph_sym_normalize", 3.0 * nnz, 16.0 * N + 24.0 * nnz);
    DMVAE_LAUNCH(spread_degree_kernel, dim3((N + 255) / 256), dim3(256), 0, st, indptr, indices, w, N, nnz, r, err_flag);
    if (nnz > 0) DMVAE_LAUNCH(spread_scale_kernel, dim3((int)(((int64_t)N * 8 + 255) / 256)), dim3(256), 0, st, indptr, indices, w, N, nnz, r, s);
    return check_launch(who);
}

int label_spread_launch(hipStream_t st, const int64_t* indptr, const int32_t* indices, const float* s, int N, int64_t nnz, const int32_t* labels, int C,
                        float alpha, int n_iter, const float* F_in, int64_t ld_in, float* F, int64_t ldf, float* change, void* ws, int64_t ws_bytes,
                        int32_t* err_flag) {
    const char* who = "dmvae_label_spread";
    SPREAD_REQUIRE(N >= 1 && N <= SPREAD_MAX_N, "%s: N=%d (1 .. %d)", who, N, SPREAD_MAX_N);
    SPREAD_REQUIRE(C >= SPREAD_MIN_C && C <= SPREAD_MAX_C, "%s: C=%d (%d .. %d)", who, C, SPREAD_MIN_C, SPREAD_MAX_C);
    SPREAD_REQUIRE(nnz >= 0, "%s: nnz=%lld (>= 0)", who, (long long)nnz);
    SPREAD_REQUIRE(n_iter >= 1, "%s: n_iter=%d (>= 1)", who, n_iter);
    SPREAD_REQUIRE(alpha > 0.f && alpha < 1.f, "%s: alpha=%g (0 < alpha < 1)", who, (double)alpha);
    SPREAD_REQUIRE(indptr && labels && F && change && err_flag, "%s: null indptr / labels / F / change / err_flag", who);
    SPREAD_REQUIRE(nnz == 0 || (indices && s), "%s: null indices / s with nnz=%lld", who, (long long)nnz);
    SPREAD_REQUIRE(ldf >= C, "%s: ldf=%lld < C=%d", who, (long long)ldf, C);
    SPREAD_REQUIRE(!F_in || ld_in >= C, "%s: ld_in=%lld < C=%d", who, (long long)ld_in, C);
    const int64_t need = label_spread_ws_bytes(N, C);
    SPREAD_REQUIRE(ws && ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (dmvae_label_spread_ws_bytes)", who, (long long)ws_bytes, (long long)need);
    SPREAD_REQUIRE((uintptr_t)ws % 16 == 0, "%s: workspace not 16-byte aligned", who);

    const SpreadShape h = spread_shape(C);
    const int64_t nw = spread_n_waves(N, C);
    char* base = (char*)ws;
    float* buf[2] = {(float*)base, (float*)(base + align256((int64_t)N * h.Cp * 4))};
    unsigned int* part0 = (unsigned int*)(base + 2 * align256((int64_t)N * h.Cp * 4));
    unsigned int* part[2] = {part0, (unsigned int*)((char*)part0 + align256(nw * 4))};
    // n_iter = 1 with F_in inside the caller's F: the launch may not write the rows other workgroups still read
    const char *fb = (const char*)F, *fe = fb + ((int64_t)(N - 1) * ldf + C) * 4;
    const char *ib = (const char*)F_in, *ie = ib + ((int64_t)(N - 1) * ld_in + C) * 4;
    const bool in_place = F_in && ib < fe && fb < ie;
    const bool unpack = n_iter == 1 && in_place;

    SpreadArgs a{};
    a.indptr = indptr; a.indices = indices; a.s = s; a.labels = labels;
    a.N = N; a.C = C; a.nch = h.nch; a.G = h.G; a.npass = h.npass; a.nnz = nnz;
    a.gshift = 0;
    while ((1 << a.gshift) < h.G) ++a.gshift;
    a.alpha = alpha; a.beta = (float)(1.0 - (double)alpha);
    a.err = err_flag;
    const double fl = 2.0 * (double)nnz * C, by = (double)nnz * (8.0 + 4.0 * h.Cp) + 12.0 * N * h.Cp;
    ProfScope ps(st, "label_spread", fl * n_iter, by * n_iter);
    const float* src = F_in;
    int64_t ld_src = ld_in;
    int v_src = F_in && ld_in >= h.Cp && ld_in % 4 == 0 && (uintptr_t)F_in % 16 == 0;
    for (int t = 0; t < n_iter; ++t) {
        const bool last = t == n_iter - 1 && !unpack;
        a.fin = src; a.ldin = ld_src; a.vin = v_src;
        a.fout = last ? F : buf[t & 1]; a.ldout = last ? ldf : h.Cp; a.vout = last ? 0 : 1;
        a.part = part[t & 1];
        a.part_prev = t ? part[(t - 1) & 1] : nullptr; a.n_prev = (int)nw; a.change_prev = t ? change + (t - 1) : nullptr;
        const dim3 grid((int)(nw / SPREAD_WAVES)), block(64 * SPREAD_WAVES);
        if (!a.fin) DMVAE_LAUNCH(spread_iter_kernel<SPREAD_IN_ZERO>, grid, block, 0, st, a);
        else if (a.vin) DMVAE_LAUNCH(spread_iter_kernel<SPREAD_IN_VEC>, grid, block, 0, st, a);
        else DMVAE_LAUNCH(spread_iter_kernel<SPREAD_IN_SCALAR>, grid, block, 0, st, a);
        src = a.fout; ld_src = a.ldout; v_src = a.vout;
    }
    DMVAE_LAUNCH(spread_join_kernel, dim3(1), dim3(64 * SPREAD_WAVES), 0, st, part[(n_iter - 1) & 1], (int)nw, change + (n_iter - 1));
    if (unpack) DMVAE_LAUNCH(spread_unpack_kernel, dim3((int)(((int64_t)N * C + 255) / 256)), dim3(256), 0, st, buf[0], (int64_t)h.Cp, F, ldf, N, C);
    return check_launch(who);
}

}  // namespace dmvae
