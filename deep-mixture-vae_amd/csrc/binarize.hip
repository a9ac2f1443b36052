// Binarisation of rows on the device: out[r][c] = (u(r, c) < x[r][c]) ? 1 : 0 for rows X [n_rows][ldx] (f32, n_cols used) into out [n_rows][ldo].
//   mode BINARIZE_BERNOULLI  u = philox_uniform_at(seed, counter, stream 8, idx),  idx = (row_base + r) * n_cols + c  in 64 bits: word idx & 3 of block
//                            idx >> 2, the exact grid (w >> 8) * 2^-24 in [0, 1) -- x = 0 (and anything below) never fires, x >= 1 always fires.
//                            row_base is the row's index in the unpermuted data set, so the draw is a function of (seed, counter, data-set row, column)
//                            alone: batch size, row order, rank count and chunked calls do not enter.
//   mode BINARIZE_THRESHOLD  x > 0.5f, no noise read.
// A NaN compares false and gives 0 in both modes.
//   binarize_rows_kernel     one Philox block feeds four consecutive FLAT indices, so a lane owns aligned groups of four flat indices and calls philox_block
//                            once per group.  With n_cols a multiple of 4 a group is four columns of one row; otherwise groups straddle rows, and the
//                            first and last group of a call may reach into rows the call does not hold: a group finds (row, column) of its first
//                            element by ONE 64-bit division and walks on from there.  A group that lies inside one row loads / stores its 16 bytes
//                            at once where the address allows (row offset and ld decide, per side), scalars otherwise; pad columns c >= n_cols of out
//                            are never written.  Grid-stride over the groups, no LDS, no atomics: 8 bytes per element, bandwidth-bound.
#include "binarize.h"

namespace dmvae {

struct BinarizeArgs {
    const float* X; int64_t ldx;
    float* out; int64_t ldo;
    int64_t total, n_groups;                     // n_rows * n_cols elements in n_groups groups of four flat indices
    uint64_t first_group; int head;              // flat index of the call's first element = 4 * first_group + head
    int n_cols, mode;
    uint64_t seed, counter;
};

__device__ __forceinline__ float binarize_fire(float x, uint32_t w, int mode) {
    const float t = mode == BINARIZE_THRESHOLD ? 0.5f : (float)(w >> 8) * (1.0f / 16777216.0f);
    return t < x ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void binarize_rows_kernel(BinarizeArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < a.n_groups; k += stride) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (a.mode == BINARIZE_BERNOULLI) philox_block(a.seed, a.counter, BINARIZE_PHILOX_STREAM, a.first_group + (uint64_t)k, w);
        const int64_t l0 = 4 * k - a.head;                        // the call's own flat index of the group's element 0 (< 0: before its first row)
        const int j0 = l0 < 0 ? (int)-l0 : 0;
        const int j1 = a.total - l0 < 4 ? (int)(a.total - l0) : 4;
        const uint64_t lf = (uint64_t)(l0 + j0);
        int64_t r = (int64_t)(lf / (uint32_t)a.n_cols);
        int c = (int)(lf - (uint64_t)r * (uint32_t)a.n_cols);
        const float* x = a.X + r * a.ldx + c;
        float* o = a.out + r * a.ldo + c;
        if (j0 == 0 && j1 == 4 && c + 4 <= a.n_cols) {           // four columns of one row
            float v[4];
            if (((uintptr_t)x & 15) == 0) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(x);
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            } else {
                v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
            }
            const f32x4 y = {binarize_fire(v[0], w[0], a.mode), binarize_fire(v[1], w[1], a.mode), binarize_fire(v[2], w[2], a.mode),
                             binarize_fire(v[3], w[3], a.mode)};
            if (((uintptr_t)o & 15) == 0) {
                *reinterpret_cast<f32x4*>(o) = y;
            } else {
                o[0] = y[0]; o[1] = y[1]; o[2] = y[2]; o[3] = y[3];
            }
        } else {                                                  // a ragged edge: element by element, across the end of a row
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= j0 && j < j1) {
                    *o = binarize_fire(*x, w[j], a.mode);
                    ++x; ++o;
                    if (++c == a.n_cols) { c = 0; ++r; x = a.X + r * a.ldx; o = a.out + r * a.ldo; }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define BINARIZE_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int binarize_rows_launch(hipStream_t s, const float* X, int64_t ldx, int64_t n_rows, int n_cols, int64_t row_base, uint64_t seed, uint64_t counter,
                         int mode, float* out, int64_t ldo) {
    const char* who = "dmvae_binarize_rows";
    BINARIZE_REQUIRE(X && out, "%s: null X / out", who);
    BINARIZE_REQUIRE(n_rows >= 1 && n_cols >= 1, "%s: n_rows=%lld, n_cols=%d (n_rows >= 1, n_cols >= 1)", who, (long long)n_rows, n_cols);
    BINARIZE_REQUIRE(ldx >= n_cols && ldo >= n_cols, "%s: ldx=%lld, ldo=%lld (ldx >= n_cols, ldo >= n_cols)", who, (long long)ldx, (long long)ldo);
    BINARIZE_REQUIRE(row_base >= 0, "%s: row_base=%lld (row_base >= 0)", who, (long long)row_base);
    BINARIZE_REQUIRE(mode == BINARIZE_BERNOULLI || mode == BINARIZE_THRESHOLD, "%s: mode=%d (0: Bernoulli draw, 1: threshold)", who, mode);
    typedef unsigned __int128 u128;
    const u128 flat_end = ((u128)row_base + (u128)n_rows) * (u128)n_cols;
    BINARIZE_REQUIRE(flat_end < (u128)BINARIZE_MAX_FLAT, "%s: (row_base + n_rows) * n_cols = (%lld + %lld) * %d reaches 2^58: the block index would enter the stream bits",
                     who, (long long)row_base, (long long)n_rows, n_cols);
    // the byte spans of the two sides, first element to last; a span past the address space cannot be a buffer
    const u128 xb = (u128)(uintptr_t)X, ob = (u128)(uintptr_t)out;
    const u128 xe = xb + 4 * ((u128)(n_rows - 1) * (u128)ldx + (u128)n_cols), oe = ob + 4 * ((u128)(n_rows - 1) * (u128)ldo + (u128)n_cols);
    BINARIZE_REQUIRE(xe <= ((u128)1 << 64) && oe <= ((u128)1 << 64), "%s: rows of ldx=%lld / ldo=%lld do not fit the address space", who, (long long)ldx,
                     (long long)ldo);
    BINARIZE_REQUIRE(xe <= ob || oe <= xb, "%s: out overlaps X (the spans of the two sides, first element to last, must be disjoint)", who);

    const int64_t total = n_rows * n_cols, flat0 = row_base * n_cols;
    const int head = (int)(flat0 & 3);
    const int64_t n_groups = (head + total + 3) >> 2;
    const int64_t want = (n_groups + 255) / 256;
    const int nb = (int)(want < 2048 ? want : 2048);             // 8 blocks on each of the 256 CUs; the loop strides over the rest
    ProfScope ps(s, "binarize_rows", 0.0, 8.0 * (double)total);
    const BinarizeArgs a{X, ldx, out, ldo, total, n_groups, (uint64_t)flat0 >> 2, head, n_cols, mode, seed, counter};
    DMVAE_LAUNCH(binarize_rows_kernel, dim3(nb), dim3(256), 0, s, a);
    return check_launch(who);
}

}  // namespace dmvae
