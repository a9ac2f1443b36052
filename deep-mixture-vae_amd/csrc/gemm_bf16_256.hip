// 256x256 macro-tile bf16 MFMA GEMM for gfx950 -- the large dense layers (M, N >= 2048: the 4096-wide
// stack of BASELINE.json's configs[4], the 4096-column [z|c]-hidden layer of the MNIST-shaped configs).
// Same three operand layouts and fused epilogues as gemm_bf16.hip (tf.layers.dense forward / dX / dW of
// code/base_models.py:221-248,279-293 and their tf.gradients, :110).
//
// Why a second kernel: the 64..128-wide tiles of gemm_bf16.hip run at the CU's L2 -> LDS intake (~70 GB/s per CU,
// DESIGN.md section 6); a 128x128 tile gives 64 flop per intake byte = a ~1.15 PFLOP/s ceiling.  A 256x256 tile
// gives 128 flop/B.  It needs 128 KiB of LDS, so there is ONE workgroup per CU, and the load / compute overlap that
// two resident workgroups gave has to happen INSIDE the workgroup:
//
//   * 8 waves = 2 (M) x 4 (N); wave (wr, wc) owns rows {ai*128 + wr*64 + 0..63 : ai = 0, 1} x cols wc*64 + 0..63
//     (32 accumulator tiles of 16x16 = 128 VGPRs).  Waves w and w + 4 share a SIMD.
//   * a K tile (64 deep) is FOUR half-tiles of 16 KiB: A-lo, B-lo, B-hi, A-hi (128 rows / columns each); LDS holds two
//     K tiles (8 half-tile buffers).  One K tile = four PHASES per wave; phase p = the 16 MFMAs of one quadrant
//     (64 rows x 32 cols x 64 k) behind the LDS fragment reads it needs:
//         p0: read a <- A-lo (8 fragments), b0 <- B (4)   Q(0,0)        p2: read a <- A-hi (8)   Q(1,1)
//         p1: read b1 <- B (4)                           Q(0,1)        p3: (b0 still in registers) Q(1,0)
//     so A-hi is not needed before p2, and every phase issues ONE half-tile of LDS-DMA (2 instructions per wave),
//     LOOKAHEAD = 6 half-tiles (96 KiB) ahead of its consumption.
//   * the two wave groups (wr = 0 / wr = 1) run STAGGERED by one barrier: a phase is
//         [fragment reads, DMA issue, counted vmcnt]  s_barrier  [16 MFMAs]  s_barrier
//     and group 1 executes one extra barrier up front, so in every barrier interval one wave of each SIMD multiplies
//     while its partner reads / issues / waits -- the matrix pipe of every SIMD alternates between its two waves.
//
// Hazards (g = global barrier count; group 0's phase q sits between barriers 2q-1 .. 2q+1, group 1's one later):
//   RAW  half-tile s (stream order A-lo, B-lo, B-hi, A-hi per K tile) is first read in phase c(s) >= s - 2 (B-hi of
//        tile t: c = 4t = s - 2).  Every wave retires its share of s with vmcnt in phase s - 3 BEFORE that phase's
//        first barrier; both groups have passed that barrier before any read of phase s - 2 starts.  After the
//        wait LOOKAHEAD - 3 half-tiles stay in flight: s_waitcnt vmcnt(6).
//   WAR  s overwrites the buffer of s - 8, last read in phase c' <= s - 8; it is issued in phase s - 6, and the
//        reads of phase c' are complete (lgkmcnt(0) in front of the MFMAs) before group 1 passes barrier 2c' + 2,
//        which group 0 passes before its phase c' + 2 = s - 6 issues.
//   The last 6 issues of a tile run past the K range: they re-load the last K tile into buffers nobody reads again
//   (keeps the vmcnt arithmetic uniform; 96 KiB of L2 hits per 256x256 tile).
// Epilogue: every wave parks a 64x64 fp32 block in its PRIVATE 16 KiB of the idle LDS (XOR-swizzled, conflict-free)
// and re-reads it row-contiguous: 128..256-byte row segments per 16 lanes -> the fused epilogues of
// gemm_epilogue.h, or the TF-Adam update on the gradient quad (DMVAE_EPI_ADAM).
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "gemm_tile.h"
#include "measure.h"      // MEAS_*: empty in the product build

namespace dmvae {

// (tools/anatomy256.py, tools/clock256.py -- measure.h: the clock the chip holds in the K loop is (slot 5 - slot 4) / (slot 1 - slot 0) x 100 MHz)
MEAS_TABLES_256
constexpr int HALF_ELEMS = 128 * BK;     // one half-tile: 128 rows (or columns) x 64 k of bf16 = 16 KiB
constexpr int LOOKAHEAD = 6;             // half-tiles issued ahead of the phase that consumes them
#ifndef DMVAE_ADAM256_NB
#define DMVAE_ADAM256_NB 4
#define DMVAE_ADAM256_DEPTH 2
#endif
constexpr int ADAM_NB = DMVAE_ADAM256_NB, ADAM_DEPTH = DMVAE_ADAM256_DEPTH;               // quads per batch of the dW + Adam epilogue; two batches of parameter / m / v loads in flight (adam_pipelined)
template <int V> using IC = std::integral_constant<int, V>;

// Bias gradient of a dW problem: db[n] = sum_k dY[k][n].  The smaller tiles get it from a ones-operand MFMA in the
// first tile row (gemm_bf16.hip); with ONE 256x256 tile per CU that would make a sixteenth of the tiles 12 % longer
// and the whole launch with them.  Here: colsum_slabs_kernel sums 64 row slabs of dY (16-B loads, fixed order) into
// part[slab][n]; the dW launch's extra workgroups add the slabs in ascending order and store db / apply its Adam.
struct BiasSeg {
    const float* part; int nslab; int n;      // part[nslab][n]
    float* out;                               // db in the gradient arena (ADAM: locates the arena offset; written only when store_grad)
};

// up to COLSUM_MAX problems (same row count) in one launch: the column blocks of problem i are blockIdx.x in [xb[i], xb[i + 1])
constexpr int COLSUM_MAX = 4;
struct ColsumBatch {
    int n, rows, rows_per_slab;
    int xb[COLSUM_MAX + 1];
    const bf16_t* in[COLSUM_MAX]; int64_t ld[COLSUM_MAX]; int N[COLSUM_MAX]; float* part[COLSUM_MAX];
};
__global__ __launch_bounds__(256) void colsum_slabs_kernel(ColsumBatch cb) {
    __shared__ float red[4][512 + 8];
    int pi = 0;
    while (pi + 1 < cb.n && (int)blockIdx.x >= cb.xb[pi + 1]) ++pi;
    const bf16_t* in = cb.in[pi]; const int64_t ld = cb.ld[pi]; const int rows = cb.rows, rows_per_slab = cb.rows_per_slab, N = cb.N[pi];
    float* part = cb.part[pi];
    const int bx = (int)blockIdx.x - cb.xb[pi];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = bx * 512 + lane * 8;
    const int r0 = blockIdx.y * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (n < N)
#pragma unroll 8
        for (int r = r0 + wave; r < r1; r += 4) {      // (unrolled: eight 16-byte loads in flight per lane)
            const uint4 q = *reinterpret_cast<const uint4*>(in + (int64_t)r * ld + n);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[2 * j] += __uint_as_float(w[j] << 16);
                s[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u);
            }
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave][lane * 8 + j] = s[j];
    __syncthreads();
    for (int c = threadIdx.x; c < 512; c += 256)
        if (bx * 512 + c < N)
            part[(int64_t)blockIdx.y * N + bx * 512 + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// bias gradient from its partials (slab column sums, or the per-tile column sums dY's producer left) + its Adam update:
// workgroup e of ne (512 threads each)
template <int EPI>
__device__ __forceinline__ void bias_seg_block(const BiasSeg& bs, const dmvae_adam_ctx& ac, const int e, const int ne) {
    for (int q = e * 512 + (int)threadIdx.x; q < bs.n / 4; q += ne * 512) {
        float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int sl = 0; sl < bs.nslab; ++sl) {                      // ascending order
            const float4 p4 = *reinterpret_cast<const float4*>(bs.part + (int64_t)sl * bs.n + 4 * q);
            g4.x += p4.x; g4.y += p4.y; g4.z += p4.z; g4.w += p4.w;
        }
        if constexpr (EPI == DMVAE_EPI_ADAM) {
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
            adam_quad(ac, (bs.out - ac.grad) + 4 * q, gv);
        } else {
            *reinterpret_cast<float4*>(bs.out + 4 * q) = g4;
        }
    }
}

// one 256x256 output tile; bid = tile id within the problem (the caller did the XCD-aware remap)
template <int LAYOUT, int EPI>
// kslice >= 0 (DW layout, STORE_F32, GemmArgs::k_split < K): the tile's K range is [kslice * k_split, (kslice + 1) * k_split) and its
// partial product goes to slab kslice (out + kslice * slab_stride): deterministic split-K, the slabs are added in a fixed order later
__device__ __forceinline__ void gemm256_tile(const GemmArgs& a, const dmvae_adam_ctx& ac, const int bid, bf16_t* smem, const int kslice = -1) {
    // (scalars, not a modified copy of the argument block: the LDS-DMA takes its tile pointer from SGPRs)
    int kdim = a.K;
    int64_t koffA = 0, koffB = 0, slab_off = 0;
    if constexpr (LAYOUT == DMVAE_GEMM_DW && EPI == DMVAE_EPI_STORE_F32) {
        if (kslice >= 0) {           // both operands are [K][..] in this layout: the slice is a row offset
            kdim = a.k_split;
            koffA = (int64_t)kslice * a.k_split * a.lda;
            koffB = (int64_t)kslice * a.k_split * a.ldb;
            slab_off = (int64_t)kslice * a.slab_stride;
        }
    }
    constexpr bool A_KC = (LAYOUT != DMVAE_GEMM_DW);
    constexpr bool B_KC = (LAYOUT == DMVAE_GEMM_DX);
    MEAS_ANAT256(0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    // tiles of an XCD's run are walked in supertiles, as in gemm_bf16.hip
    const int tiles_n = a.N / 256, tiles_m = a.M / 256;
    int tm, tn;
    {
        const int gm_max = a.group_m;
        const int gsz = gm_max * tiles_n, grp = bid / gsz, first = grp * gm_max;
        const int gm = min(tiles_m - first, gm_max), in = bid - grp * gsz;
        tm = first + in % gm;
        tn = in / gm;
    }
    const int m0 = tm * 256, n0 = tn * 256;
    const int nk = kdim / BK;

    const bf16_t* Ag = reinterpret_cast<const bf16_t*>(a.A) + koffA + (A_KC ? (int64_t)m0 * a.lda : (int64_t)m0);
    const bf16_t* Bg = reinterpret_cast<const bf16_t*>(a.B) + koffB + (B_KC ? (int64_t)n0 * a.ldb : (int64_t)n0);
    const int64_t stepA = A_KC ? (int64_t)BK : (int64_t)BK * a.lda;
    const int64_t stepB = B_KC ? (int64_t)BK : (int64_t)BK * a.ldb;
    const int64_t hiA = A_KC ? (int64_t)128 * a.lda : (int64_t)128;     // A-hi relative to A-lo
    const int64_t hiB = B_KC ? (int64_t)128 * a.ldb : (int64_t)128;

    // loop-invariant per-lane addressing
    unsigned goA[2], goB[2];
    stage_offsets<128, A_KC, 8, BK>(a.lda, wave, lane, goA);
    stage_offsets<128, B_KC, 8, BK>(a.ldb, wave, lane, goB);
    unsigned foA[4], foB[4];             // fragment offsets of K sub-step 0; sub-step 1 and the second transposing read: read_frag_ks
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned short lo, hi;
        frag_offsets<128, A_KC>(wr * 64 + i * 16, 0, lane, lo, hi);
        foA[i] = lo;
        frag_offsets<128, B_KC>((wc & 1) * 64 + i * 16, 0, lane, lo, hi);
        // this wave's B half (columns wc*64.. lie in B-lo for wc < 2, in B-hi else) is folded into the offsets
        foB[i] = (unsigned)lo + (unsigned)((wc >> 1) * HALF_ELEMS);
    }
    const unsigned lds_w = __builtin_amdgcn_readfirstlane(
        (unsigned)(size_t)((__attribute__((address_space(3))) bf16_t*)smem) + 1024u * (unsigned)wave);

    f32x4 acc[2][4][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // LDS-DMA of half-tile J (stream order: 0 A-lo, 1 B-lo, 2 B-hi, 3 A-hi) of K tile ts into the buffers of parity PAR
    auto issue = [&](auto Jc, auto PARc, int ts) {
        constexpr int J = decltype(Jc)::value, PAR = decltype(PARc)::value;
        const int tc = ts < nk ? ts : nk - 1;
        constexpr unsigned buf = 2u * (unsigned)((PAR * 4 + (J == 0 ? 0 : J == 3 ? 1 : J == 1 ? 2 : 3)) * HALF_ELEMS);
        if constexpr (J == 0) glds_tile(Ag + tc * stepA, goA, lds_w + buf, 8192u);
        else if constexpr (J == 3) glds_tile(Ag + hiA + tc * stepA, goA, lds_w + buf, 8192u);
        else if constexpr (J == 1) glds_tile(Bg + tc * stepB, goB, lds_w + buf, 8192u);
        else glds_tile(Bg + hiB + tc * stepB, goB, lds_w + buf, 8192u);
    };

    bf16x8 fa[4][2], fb0[2][2], fb1[2][2];
    // one phase of K tile t (buffer parity PAR): reads, DMA issue, counted wait | barrier | 16 MFMAs | barrier
    auto phase = [&](auto Pc, auto PARc, int t) {
        constexpr int P = decltype(Pc)::value, PAR = decltype(PARc)::value;
        const bf16_t* At = smem + (PAR * 4 + (P >= 2 ? 1 : 0)) * HALF_ELEMS;
        const bf16_t* Bt = smem + (PAR * 4 + 2) * HALF_ELEMS;
        if constexpr (P == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                { fb0[j][0] = read_frag_ks<128, B_KC, 0>(Bt, foB[j]); fb0[j][1] = read_frag_ks<128, B_KC, 1>(Bt, foB[j]); }
        }
        if constexpr (P == 1) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                { fb1[j][0] = read_frag_ks<128, B_KC, 0>(Bt, foB[2 + j]); fb1[j][1] = read_frag_ks<128, B_KC, 1>(Bt, foB[2 + j]); }
        }
        if constexpr (P == 0 || P == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                { fa[i][0] = read_frag_ks<128, A_KC, 0>(At, foA[i]); fa[i][1] = read_frag_ks<128, A_KC, 1>(At, foA[i]); }
        }
        // half-tile (4t + P) + LOOKAHEAD: J = (P + 2) & 3 of K tile t + 1 (P < 2) / t + 2 (P >= 2)
        issue(IC<(P + 2) & 3>{}, IC<(P < 2 ? 1 - PAR : PAR)>{}, t + (P < 2 ? 1 : 2));
        wait_vmcnt<2 * (LOOKAHEAD - 3)>();
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        constexpr int AI = P >= 2 ? 1 : 0;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // operands swapped (D[row = n][col = m]): a lane owns 4 consecutive n of one m
                    if constexpr (P == 0 || P == 3)
                        acc[AI][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb0[j][ks], fa[i][ks], acc[AI][i][j], 0, 0, 0);
                    else
                        acc[AI][i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb1[j][ks], fa[i][ks], acc[AI][i][2 + j], 0, 0, 0);
                }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    };

    // prologue: half-tiles 0..5 (K tile 0 whole, A-lo and B-lo of K tile 1); A-lo, B-lo, B-hi of tile 0 landed
    issue(IC<0>{}, IC<0>{}, 0); issue(IC<1>{}, IC<0>{}, 0); issue(IC<2>{}, IC<0>{}, 0); issue(IC<3>{}, IC<0>{}, 0);
    issue(IC<0>{}, IC<1>{}, 1); issue(IC<1>{}, IC<1>{}, 1);
    wait_vmcnt<2 * (LOOKAHEAD - 3)>();
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();       // the stagger: group 1 runs one barrier behind group 0
    for (int t = 0; t < nk; t += 2) {
        phase(IC<0>{}, IC<0>{}, t); phase(IC<1>{}, IC<0>{}, t); phase(IC<2>{}, IC<0>{}, t); phase(IC<3>{}, IC<0>{}, t);
        if (t + 1 < nk) {
            phase(IC<0>{}, IC<1>{}, t + 1); phase(IC<1>{}, IC<1>{}, t + 1); phase(IC<2>{}, IC<1>{}, t + 1); phase(IC<3>{}, IC<1>{}, t + 1);
        }
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();       // pairs with group 1's last barrier
    wait_vmcnt<0>();                                 // the trailing re-loads: every DMA write has landed ...
    __builtin_amdgcn_s_barrier();                    // ... for every wave, before LDS is reused
    MEAS_ANAT256(1);

    // ---- epilogue: two 64 x 64 fp32 blocks per wave through the wave's private 16 KiB
    float loss = 0.f;
    float* st = reinterpret_cast<float*>(smem) + wave * 4096;
    const int li = lane & 15, g = lane >> 4;
    constexpr bool CSUM = (EPI == DMVAE_EPI_RELU_MASK || EPI == DMVAE_EPI_BIAS_RECON);     // the output is a dY: its column sums = a bias gradient
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr bool HAS_BIAS = (EPI == DMVAE_EPI_BIAS_RELU || EPI == DMVAE_EPI_BIAS_F32 || EPI == DMVAE_EPI_BIAS_SIGMOID || EPI == DMVAE_EPI_BIAS_RECON);
    float bq[4] = {0.f, 0.f, 0.f, 0.f};         // a lane's column quad is the same for every row it handles: the bias once
    if constexpr (HAS_BIAS) loadf4(a.epi.bias, n0 + wc * 64 + li * 4, bq);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = i * 16 + li, c = j * 4 + g;
                *reinterpret_cast<f32x4*>(st + r * 64 + ((c ^ (r & 7)) << 2)) = acc[h][i][j];
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // same wave, in-order LDS: the block is written
        if constexpr (EPI == DMVAE_EPI_ADAM) {                  // batches of ADAM_NB quads: loads of a batch in flight together (adam_quads)
            const unsigned base = (unsigned)((reinterpret_cast<const float*>(a.epi.out) - ac.grad) + (int64_t)(m0 + h * 128 + wr * 64) * a.epi.ldo + n0 + wc * 64 + li * 4);
            adam_pipelined<ADAM_NB, 16 / ADAM_NB, ADAM_DEPTH>(ac,
                [&](int i, int b) { return base + (unsigned)((i * ADAM_NB + b) * 4 + g) * (unsigned)a.epi.ldo; },
                [&](int i, int b, float (&gv)[4]) {
                    const int r = (i * ADAM_NB + b) * 4 + g;
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(st + r * 64 + ((li ^ (r & 7)) << 2));
                    gv[0] = t4[0]; gv[1] = t4[1]; gv[2] = t4[2]; gv[3] = t4[3];
                });
        } else {
            // batches of EPI_NB rows: the gate / target loads of a batch are issued before its first store (see epilogue_quad)
            constexpr int EPI_NB = 8;
#pragma unroll 1
            for (int it0 = 0; it0 < 16; it0 += EPI_NB) {
                float pre[EPI_NB][4];
                if constexpr (EPI == DMVAE_EPI_RELU_MASK || EPI == DMVAE_EPI_BIAS_RECON) {
#pragma unroll
                    for (int b = 0; b < EPI_NB; ++b) {
                        const int64_t o = (int64_t)(m0 + h * 128 + wr * 64 + (it0 + b) * 4 + g) * a.epi.ld0 + n0 + wc * 64 + li * 4;
                        if constexpr (EPI == DMVAE_EPI_RELU_MASK) ActIO<bf16_t>::load4(a.epi.aux0, o, pre[b]);
                        else loadf4(a.epi.aux0, o, pre[b]);
                    }
                }
#pragma unroll
                for (int b = 0; b < EPI_NB; ++b) {
                    const int r = (it0 + b) * 4 + g, c = li;
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(st + r * 64 + ((c ^ (r & 7)) << 2));
                    float v[4] = {t4[0], t4[1], t4[2], t4[3]};
                    const int m = m0 + h * 128 + wr * 64 + r, n = n0 + wc * 64 + c * 4;
                    if constexpr (CSUM) {
                        float sv[4];
                        epilogue_quad<EPI, bf16_t>(a.epi, m, n, v, loss, EPI == DMVAE_EPI_BIAS_RECON ? pre[b] : nullptr, sv, HAS_BIAS ? bq : nullptr,
                                                   EPI == DMVAE_EPI_RELU_MASK ? pre[b] : nullptr);
#pragma unroll
                        for (int j = 0; j < 4; ++j) cs[j] += bf2f(f2bf(sv[j]));       // the value the weight-gradient GEMM will read
                    } else if constexpr (EPI == DMVAE_EPI_STORE_F32) {       // (K slice: its slab)
                        ActIO<float>::store4(reinterpret_cast<float*>(a.epi.out) + slab_off, (int64_t)m * a.epi.ldo + n, v);
                    } else {
                        epilogue_quad<EPI, bf16_t>(a.epi, m, n, v, loss, nullptr, nullptr, HAS_BIAS ? bq : nullptr);
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the next block overwrites
    }
    if constexpr (CSUM) {
        if (a.csum_out) {     // fixed order: a lane's rows ascending, the 4 row classes (shuffles), then wave row 0 + wave row 1
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cs[j] += __shfl_xor(cs[j], 16, 64);
                cs[j] += __shfl_xor(cs[j], 32, 64);
            }
            __syncthreads();                                   // every wave is done with its staging block
            float* cx = reinterpret_cast<float*>(smem);        // [4 wave columns][64]
            if (wr == 1 && g == 0) *reinterpret_cast<float4*>(cx + wc * 64 + li * 4) = make_float4(cs[0], cs[1], cs[2], cs[3]);
            __syncthreads();
            if (wr == 0 && g == 0) {
                const float4 o4 = *reinterpret_cast<const float4*>(cx + wc * 64 + li * 4);
                *reinterpret_cast<float4*>(a.csum_out + (int64_t)tm * a.csum_ld + n0 + wc * 64 + li * 4) =
                    make_float4(cs[0] + o4.x, cs[1] + o4.y, cs[2] + o4.z, cs[3] + o4.w);
            }
        }
    }
    if constexpr (EPI == DMVAE_EPI_BIAS_RECON) {
        float* red = reinterpret_cast<float*>(smem);
        __syncthreads();
        const float t = block_sum_waves<8>(loss, red);
        if (tid < 16) a.epi.partials[(tm * 4 + tid / 4) * (a.N / 64) + tn * 4 + tid % 4] = tid == 0 ? t : 0.f;   // 64x64 cell grid, see gemm_bf16.hip
    }
    MEAS_ANAT256_DRAIN();
}

template <int LAYOUT, int EPI>
__global__ __launch_bounds__(512, 2) void gemm_bf16_256_kernel(GemmArgs a, dmvae_adam_ctx ac, int ntiles, BiasSeg bs) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[8 * HALF_ELEMS];       // 128 KiB: 2 K tiles x {A-lo, A-hi, B-lo, B-hi}
    if constexpr (LAYOUT == DMVAE_GEMM_DW) {
        if ((int)blockIdx.x >= ntiles) {         // extra workgroups: the bias gradient
            bias_seg_block<EPI>(bs, ac, (int)blockIdx.x - ntiles, (int)gridDim.x - ntiles);
            return;
        }
    }
    // XCD-aware tile order: a contiguous run of tile ids per XCD
    gemm256_tile<LAYOUT, EPI>(a, ac, xcd_run_index((int)blockIdx.x, 0, ntiles), smem);
}

// Several weight-gradient problems in ONE grid (the 4096-wide configuration has nine of 256..512 tiles each).  A launch per
// problem ends with every CU in its Adam epilogue at the same time (1.66 MB per tile: the chip's HBM rate, 80 us, with the
// matrix cores idle) and re-synchronises all CUs at every boundary.  In one grid a CU takes the next tile when it is done,
// and the first tile of every CU starts behind a delay that grows with the workgroup id: the tiles drift apart, an epilogue
// then shares HBM with few others and overlaps the other CUs' K loops.
constexpr int MULTI_MAX = 12;
struct Multi256 {
    int nprob, stagger;
    int start[MULTI_MAX + 1];            // tile workgroups of problem i: [start[i], start[i+1]) -- K slices x tiles, slice-major
    int nsl[MULTI_MAX];                  // K slices of problem i (1 = none)
    int extra[MULTI_MAX + 1];            // bias-gradient workgroups of problem i, behind all tiles: start[nprob] + [extra[i], extra[i+1])
    GemmArgs p[MULTI_MAX];
    BiasSeg bs[MULTI_MAX];
    dmvae_adam_ctx ac;
};
static_assert(sizeof(Multi256) <= 4096, "kernel argument block");
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_bf16_256_dw_multi_kernel(Multi256 m) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[8 * HALF_ELEMS];
    const int b = (int)blockIdx.x, ntile = m.start[m.nprob];
    if (b >= ntile) {
        int j = 0;
        while (j + 1 < m.nprob && b - ntile >= m.extra[j + 1]) ++j;
        bias_seg_block<EPI>(m.bs[j], m.ac, b - ntile - m.extra[j], m.extra[j + 1] - m.extra[j]);
        return;
    }
    int i = 0;
    while (i + 1 < m.nprob && b >= m.start[i + 1]) ++i;
    if (b < 256) {                       // first tile of a CU: delayed by up to `stagger` x 3.4 us, growing with the workgroup id
        const int n = (b * m.stagger) >> 8;
        for (int k = 0; k < n; ++k) __builtin_amdgcn_s_sleep(127);
    }
    int item = xcd_run_index(b, m.start[i], m.start[i + 1]), ksl = -1;
    if (m.nsl[i] > 1) {
        const int tiles_i = (m.start[i + 1] - m.start[i]) / m.nsl[i];
        ksl = item / tiles_i;
        item -= ksl * tiles_i;
    }
    gemm256_tile<DMVAE_GEMM_DW, EPI>(m.p[i], m.ac, item, smem, ksl);
}

// (A 256 x 128 weight-gradient tile on FOUR waves with an 80 KiB five-buffer half-tile ring -- TWO workgroups per CU, so that one's Adam epilogue runs
//  under the other's K loop: VERDICT r3 #1, the form DESIGN had proposed since round 2 -- was built in round 4, correct (bit-identical to this tile), and
//  21.7 % slower on the cfg5 step: 6.425 -> 7.819 ms, the launch 2.57 -> 3.69 ms = 0.78 PFLOP/s.  Without the barrier stagger of the two wave groups
//  below a wave's [fragment reads -> drain -> barrier -> 16 MFMAs] is serial and the two workgroups of a SIMD do not alternate by themselves.  Removed;
//  git history at commit aa6b3aa, numbers in profiles/r04_two_wg_dw_tile.txt, DESIGN_LOG.md R4.2.)

// ---------------------------------------------------------------- host side
void* gemm_bf16_256_anatomy() { return MEAS_SYMBOL(g_anat256); }
static int g_policy256 = 1;     // tuning knob (dmvae_debug_set_knob 6): 0 never, 1 when the grid fills the chip, 2 whenever the shape divides
void gemm_bf16_256_set_policy(int v) { g_policy256 = v; }

bool gemm_bf16_256_instantiated(int layout, int epi) {      // the pairs gemm_bf16_256_launch has
    return (layout == DMVAE_GEMM_FWD && (epi == DMVAE_EPI_BIAS_RELU || epi == DMVAE_EPI_BIAS_RECON || epi == DMVAE_EPI_STORE_F32)) ||
           (layout == DMVAE_GEMM_DX && (epi == DMVAE_EPI_RELU_MASK || epi == DMVAE_EPI_STORE_F32)) ||
           (layout == DMVAE_GEMM_DW && (epi == DMVAE_EPI_STORE_F32 || epi == DMVAE_EPI_ADAM));
}

// The 256x256 kernel takes a problem when M, N divide by 256 and the grid covers (most of) the 256 CUs; below
// that the smaller tiles' higher workgroup count wins (gemm_bf16.hip).  K >= 512: shorter K loops do not amortise
// the 6-half-tile prologue and the epilogue of a one-workgroup-per-CU tile.
bool gemm_bf16_256_ok(int layout, int epi, int M, int N, int K, bool conv) {
    if (g_policy256 == 0 || conv) return false;
    if (!gemm_bf16_256_instantiated(layout, epi) || M % 256 || N % 256 || K % BK) return false;
    if (g_policy256 == 2) return true;
    // K >= 1024: at K = 512 (the [z|c]-hidden layer of the MNIST-shaped configs) the two kernels tie (tools/gemm256_bench.py);
    // the dX of the narrow heads (K = 2 D or the padded class count) is the exception: N = 4096 columns of pure output
    // traffic, where the grouped 64x64 grid ran at 130 TFLOP/s
    const long tiles = (long)(M / 256) * (N / 256);
    return tiles >= 192 && (K >= 1024 || (layout == DMVAE_GEMM_DX && N >= 4096 && M >= 4096));
}

template <int EPI>
static int launch256_dw_multi(hipStream_t s, const GemmArgs* probs, int n, const dmvae_adam_ctx* ctx);

template <int LAYOUT, int EPI>
static int launch256(hipStream_t s, const GemmArgs& a0, const dmvae_adam_ctx* ctx) {
    GemmArgs a = a0;
    const int tiles = (a.M / 256) * (a.N / 256);
    a.group_m = gemm_auto_group_m(a.M / 256, a.N / 256, 256, 256, std::max(1.0, std::min(tiles, 256) / 8.0));
    dmvae_adam_ctx c{};
    if (ctx) c = *ctx;
    BiasSeg bs{};
    int extra = 0;
    if (LAYOUT == DMVAE_GEMM_DW && a.epi.out2 && a.csum_in) {
        // the GEMM that produced dY left its column sums per 256-row tile (GemmArgs::csum_out): nothing to re-read
        bs.part = a.csum_in; bs.nslab = a.csum_rows; bs.n = a.N; bs.out = reinterpret_cast<float*>(a.epi.out2);
        if (a.csum_ld != a.N) { set_error("gemm_bf16_256: column-sum partials must be [rows][N]"); return DMVAE_EINVAL; }
        extra = std::min(8, (a.N / 4 + 511) / 512);
    } else if (LAYOUT == DMVAE_GEMM_DW && a.epi.out2) {      // bias gradient: slab partials now, the sum (and its Adam) in the launch's extra workgroups
        float* ws = a.ws;
        int64_t ws_elems = a.ws_elems;
        if (!ws) {
            const int rc = colsum_prepare(a.N);
            if (rc) return rc;
            ws = colsum_global_scratch(&ws_elems);
        }
        constexpr int SLABS = 64;
        int rps = std::max(8, (a.K + SLABS - 1) / SLABS);
        const int nslab = (a.K + rps - 1) / rps;
        if ((int64_t)nslab * a.N > ws_elems) { set_error("gemm_bf16_256: bias-gradient scratch too small (%lld < %lld floats)", (long long)ws_elems, (long long)nslab * a.N); return DMVAE_ESTATE; }
        {
            ColsumBatch cb{};
            cb.n = 1; cb.rows = a.K; cb.rows_per_slab = rps; cb.xb[0] = 0; cb.xb[1] = (a.N + 511) / 512;
            cb.in[0] = reinterpret_cast<const bf16_t*>(a.B); cb.ld[0] = a.ldb; cb.N[0] = a.N; cb.part[0] = ws;
            ProfScope ps(s, "colsum_slabs", (double)a.K * a.N, 2.0 * a.K * a.N + 4.0 * nslab * a.N);
            DMVAE_LAUNCH(colsum_slabs_kernel, dim3(cb.xb[1], nslab), dim3(256), 0, s, cb);
        }
        bs.part = ws; bs.nslab = nslab; bs.n = a.N; bs.out = reinterpret_cast<float*>(a.epi.out2);
        extra = std::min(8, (a.N / 4 + 511) / 512);
    }
    if constexpr (LAYOUT == DMVAE_GEMM_DW && EPI == DMVAE_EPI_ADAM) {
        // a single weight-gradient problem with the fused update runs as a one-problem grid of the MERGED kernel: the single-problem
        // instantiation gemm_bf16_256_kernel<DW, ADAM> compiled to 256 VGPRs + 15 spills; the merged one is clean
        // (220-222 VGPRs) and is the one the step uses anyway.  Same tiles, same epilogue, same bits.
        if (a.epi.out2) { a.csum_in = bs.part; a.csum_rows = bs.nslab; a.csum_ld = a.N; }
        (void)extra;
        return launch256_dw_multi<DMVAE_EPI_ADAM>(s, &a, 1, ctx);
    } else {
    static const std::string nm = [] {
        char b[64];
        snprintf(b, sizeof(b), "gemm_bf16_256_kernel<%d, %d>", LAYOUT, EPI);
        return std::string(b);
    }();
    double bytes = 2.0 * ((double)a.M * a.K + (double)a.K * a.N);
    if (EPI == DMVAE_EPI_ADAM) bytes += ((double)a.M * a.N + (double)bs.n) * (24.0 + (c.param_bf16 ? 2.0 : 0.0) + (c.store_grad ? 4.0 : 0.0));
    else bytes += ((EPI == DMVAE_EPI_STORE_F32) ? 4.0 : 2.0) * a.M * a.N;
    ProfScope ps(s, nm.c_str(), 2.0 * a.M * a.N * (double)a.K, bytes);
    DMVAE_LAUNCH((gemm_bf16_256_kernel<LAYOUT, EPI>), dim3(tiles + extra), dim3(512), 0, s, a, c, tiles, bs);
    return check_launch("gemm_bf16_256");
    }
}

static int g_stagger = 0;       // tuning knob (dmvae_debug_set_knob 8): first-tile delay of the merged dW grid, units of 3.4 us spread over the 256 CUs.
                                // MEASURED at cfg5 (tools/knob_cfg5.py 8 -1 0 12 24 48): one launch per problem 7.07 ms; merged, no delay 6.89;
                                // delays 12 / 24 / 48 units 7.01 / 7.01 / 7.11 -- the tiles drift apart by themselves, a forced stagger only costs
void gemm_bf16_256_set_stagger(int v) { g_stagger = v; }      // -1: no merged grid at all (one launch per problem)

// n (2 .. MULTI_MAX) weight-gradient problems as one grid; every problem with a bias gradient must bring its column-sum partials
template <int EPI>
static int launch256_dw_multi(hipStream_t s, const GemmArgs* probs, int n, const dmvae_adam_ctx* ctx) {
    Multi256 m;
    memset(&m, 0, sizeof(m));
    m.nprob = n; m.stagger = std::max(0, g_stagger);
    if (ctx) m.ac = *ctx;
    int total = 0, extra = 0;
    double flops = 0.0, bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        GemmArgs a = probs[i];
        const int tiles = (a.M / 256) * (a.N / 256);
        const int nsl = (a.k_split > 0 && a.k_split < a.K) ? a.K / a.k_split : 1;
        if (nsl > 1 && (EPI != DMVAE_EPI_STORE_F32 || !a.slab_stride || a.epi.out2 || a.k_split % BK)) {
            set_error("gemm_bf16_256 (merged dW): K slices need the STORE_F32 epilogue into slabs and no fused bias gradient"); return DMVAE_EINVAL;
        }
        a.group_m = gemm_auto_group_m(a.M / 256, a.N / 256, 256, 256, std::max(1.0, std::min(tiles, 256) / 8.0));
        m.p[i] = a;
        m.nsl[i] = nsl;
        m.start[i] = total; total += tiles * nsl;
        m.extra[i] = extra;
        if (a.epi.out2) {
            if (!a.csum_in || a.csum_ld != a.N) { set_error("gemm_bf16_256 (merged dW): a problem with a bias gradient needs its column-sum partials"); return DMVAE_EINVAL; }
            m.bs[i].part = a.csum_in; m.bs[i].nslab = a.csum_rows; m.bs[i].n = a.N; m.bs[i].out = reinterpret_cast<float*>(a.epi.out2);
            extra += std::min(8, (a.N / 4 + 511) / 512);
        }
        flops += 2.0 * a.M * a.N * (double)a.K;
        bytes += 2.0 * ((double)a.M * a.K + (double)a.K * a.N);
        if (EPI == DMVAE_EPI_ADAM) bytes += ((double)a.M * a.N + (a.epi.out2 ? a.N : 0)) * (24.0 + (m.ac.param_bf16 ? 2.0 : 0.0) + (m.ac.store_grad ? 4.0 : 0.0));
        else bytes += 4.0 * a.M * a.N;
    }
    for (int i = n; i <= MULTI_MAX; ++i) { m.start[i] = total; m.extra[i] = extra; }
    for (int i = n; i < MULTI_MAX; ++i) m.nsl[i] = 1;
    static const std::string nm = std::string("gemm_bf16_256_dw_multi_kernel<") + std::to_string(EPI) + ">";
    ProfScope ps(s, nm.c_str(), flops, bytes);
    DMVAE_LAUNCH((gemm_bf16_256_dw_multi_kernel<EPI>), dim3(total + extra), dim3(512), 0, s, m);
    return check_launch("gemm_bf16_256_dw_multi");
}
bool gemm_bf16_256_rides() { return g_policy256 >= 1 && g_stagger >= 0; }
// K slices of a weight-gradient problem on the macro tile (partial products into slabs): the shape divides, and a slice is deep
// enough to amortise the tile's prologue / epilogue (the rule of gemm_bf16_256_ok)
bool gemm_bf16_256_slice_ok(int M, int N, int k_split) { return g_policy256 >= 1 && g_stagger >= 0 && M % 256 == 0 && N % 256 == 0 && k_split % BK == 0 && k_split >= 1024; }

// slab column sums of dY for problems whose producers left none ([nslab][N] floats each, at a.csum_in -- already pointed into the
// scratch by the caller): ONE launch for up to COLSUM_MAX problems of the same K
static int colsum_slabs_batch(hipStream_t s, GemmArgs* const* probs, int n) {
    constexpr int SLABS = 64;
    for (int lo = 0; lo < n;) {
        ColsumBatch cb{};
        const int K = probs[lo]->K;
        const int rps = std::max(8, (K + SLABS - 1) / SLABS), nslab = (K + rps - 1) / rps;
        cb.rows = K; cb.rows_per_slab = rps; cb.xb[0] = 0;
        double work = 0.0, bytes = 0.0;
        int cnt = 0;
        while (lo + cnt < n && cnt < COLSUM_MAX && probs[lo + cnt]->K == K) {
            GemmArgs& a = *probs[lo + cnt];
            cb.in[cnt] = reinterpret_cast<const bf16_t*>(a.B); cb.ld[cnt] = a.ldb; cb.N[cnt] = a.N; cb.part[cnt] = const_cast<float*>(a.csum_in);
            cb.xb[cnt + 1] = cb.xb[cnt] + (a.N + 511) / 512;
            a.csum_ld = a.N; a.csum_rows = nslab;
            work += (double)K * a.N; bytes += 2.0 * K * a.N + 4.0 * nslab * a.N;
            ++cnt;
        }
        cb.n = cnt;
        ProfScope ps(s, "colsum_slabs", work, bytes);
        DMVAE_LAUNCH(colsum_slabs_kernel, dim3(cb.xb[cnt], nslab), dim3(256), 0, s, cb);
        const int rc = check_launch("colsum_slabs");
        if (rc) return rc;
        lo += cnt;
    }
    return 0;
}

// the large weight-gradient problems of a step: merged into grids of up to MULTI_MAX, singles launched alone
int gemm_bf16_256_dw_all(hipStream_t s, const GemmArgs* probs, int n, const dmvae_adam_ctx* ctx) {
    std::vector<GemmArgs> merge;
    std::vector<size_t> need_sums;     // indices into merge: problems whose slab column sums are still to be computed
    int64_t ws_used = 0;         // the problems of one call share the caller's scratch (GemmArgs::ws): sub-allocated here
    auto flush = [&]() -> int {  // launch what has been collected (its slab sums live in [0, ws_used) of the scratch)
        if (!need_sums.empty()) {
            std::vector<GemmArgs*> ps;
            for (size_t i : need_sums) ps.push_back(&merge[i]);
            const int rc = colsum_slabs_batch(s, ps.data(), (int)ps.size());
            if (rc) return rc;
            need_sums.clear();
        }
        for (size_t lo = 0; lo < merge.size(); lo += MULTI_MAX) {
            const int cnt = (int)std::min<size_t>(MULTI_MAX, merge.size() - lo);
            int rc;
            if (cnt == 1 && merge[lo].k_split == merge[lo].K) rc = gemm_bf16_256_launch(s, DMVAE_GEMM_DW, merge[lo], ctx);
            else if (merge[lo].epi.kind == DMVAE_EPI_ADAM) rc = launch256_dw_multi<DMVAE_EPI_ADAM>(s, merge.data() + lo, cnt, ctx);
            else rc = launch256_dw_multi<DMVAE_EPI_STORE_F32>(s, merge.data() + lo, cnt, ctx);
            if (rc) return rc;
        }
        merge.clear();
        ws_used = 0;
        return 0;
    };
    for (int i = 0; i < n; ++i) {
        GemmArgs a = probs[i];
        if (a.k_split != a.K) {          // K slices into slabs: always through the merged kernel (it knows the slices), no bias gradient here
            if (a.epi.kind != DMVAE_EPI_STORE_F32 || !a.slab_stride || a.epi.out2) { set_error("gemm_bf16_256: K slices need STORE_F32 into slabs, bias gradient elsewhere"); return DMVAE_EINVAL; }
            merge.push_back(a);
            continue;
        }
        const bool has_part = a.csum_in && a.csum_ld == a.N;
        if (g_stagger < 0 || (a.epi.out2 && !has_part && (!a.ws || (int64_t)64 * a.N > a.ws_elems))) {
            // not mergeable (merging off, or a bias gradient with neither partials nor a scratch of the caller's): alone, in stream order
            int rc = flush();
            if (!rc) rc = gemm_bf16_256_launch(s, DMVAE_GEMM_DW, a, ctx);
            if (rc) return rc;
            continue;
        }
        if (a.epi.out2 && !has_part) {      // no partials from dY's producer: slab column sums now, into this problem's part of the scratch
            if (ws_used + (int64_t)64 * a.N > a.ws_elems) { const int rc = flush(); if (rc) return rc; }
            a.csum_in = a.ws + ws_used; a.csum_ld = a.N; a.csum_rows = 0;      // (rows: set by the batched launch in flush)
            ws_used += (int64_t)64 * a.N;
            need_sums.push_back(merge.size());
        }
        merge.push_back(a);
    }
    return flush();
}

int gemm_bf16_256_launch(hipStream_t s, int layout, const GemmArgs& a, const dmvae_adam_ctx* ctx) {
    const int epi = a.epi.kind;
    if (a.k_split != a.K) { set_error("gemm_bf16_256: no split-K"); return DMVAE_EINVAL; }
#define CASE256(L, E) \
    if (layout == L && epi == E) return launch256<L, E>(s, a, ctx);
    CASE256(DMVAE_GEMM_FWD, DMVAE_EPI_BIAS_RELU)
    CASE256(DMVAE_GEMM_FWD, DMVAE_EPI_BIAS_RECON)
    CASE256(DMVAE_GEMM_FWD, DMVAE_EPI_STORE_F32)
    CASE256(DMVAE_GEMM_DX, DMVAE_EPI_RELU_MASK)
    CASE256(DMVAE_GEMM_DX, DMVAE_EPI_STORE_F32)
    CASE256(DMVAE_GEMM_DW, DMVAE_EPI_STORE_F32)
    CASE256(DMVAE_GEMM_DW, DMVAE_EPI_ADAM)
#undef CASE256
    set_error("gemm_bf16_256: layout %d with epilogue %d is not instantiated", layout, epi);
    return DMVAE_EUNSUPPORTED;
}

}  // namespace dmvae
