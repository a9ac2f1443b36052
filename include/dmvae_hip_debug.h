/*
 * dmvae_hip_debug.h -- measurement and tuning entry points of libdmvae_hip.so.
 *
 * NOT part of the drop-in boundary (include/dmvae_hip.h): nothing here replaces a line of the reference.
 * bench.py's roofline leg uses dmvae_prof_* / dmvae_debug_spin; tools/ uses the probes and knobs; tests/test_gpu_conv_kernels.py
 * runs every kernel of the CNN trunk alone, on buffers of its own, through dmvae_debug_conv_* / _zero_border / _maxpool2_*;
 * tests/test_gpu_gemm_forms.py forces every tile form of the dense GEMMs through dmvae_debug_set_tile and knobs 0 / 1 / 7 / 9 (and 2 / 13 / 18),
 * checks with dmvae_prof_* which instantiation ran, and holds every fused epilogue on it to an exact reference;
 * tests/test_gpu_dw_adam_forms.py does the same for the fused weight-gradient + Adam epilogue (dmvae_gemm_grouped_dw_adam): knobs 2 and 6 (and 1)
 * force each small tile and the 256x256 macro tile alone, dmvae_prof_* says which kernel families ran and how often;
 * tests/test_gpu_step_finalize.py runs step_finalize and the batch gather in every kernel that carries them (dmvae_debug_step_finalize,
 * dmvae_debug_gemm_dx_riders, dmvae_debug_gemm_grouped_fin) and holds them, and the GEMM under them, to exact references;
 * tests/test_gpu_gemm256_forms.py does for the 256x256 macro tile what test_gpu_gemm_forms.py does for the small tiles (knob 6 = 2), and reaches the
 * arguments only the step sets -- column sums out / in, K slices into slabs -- through dmvae_debug_gemm256.
 */
#ifndef DMVAE_HIP_DEBUG_H
#define DMVAE_HIP_DEBUG_H

#include "dmvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-kernel timing with HIP events (bench.py roofline leg) ----------
 * enable(1): every launch made through this library is bracketed by a
 * hipEvent pair on its stream AND issued through hipExtLaunchKernelGGL with an
 * event pair bound to the dispatch itself.  collect() synchronises those events and
 * returns, per kernel family, launches / bracket ms / kernel ms / algorithmic flops / bytes.
 * Eager launches only (not under stream capture). */
typedef struct dmvae_prof_row {
    char name[48];
    int64_t launches;          /* profiled scopes (one per library call that launches this kernel family)       */
    double total_ms;           /* event BRACKETS around them: kernel + its dispatch / event markers              */
    double flops;   /* algorithmic */
    double bytes;   /* algorithmic */
    double kernel_ms;          /* the kernels' own begin -> end (the pair hipExtLaunchKernelGGL binds to a       */
    int64_t kernel_launches;   /* dispatch = what rocprofv3 --kernel-trace reports), and how many dispatches;    */
                               /* 0 when the runtime returned no dispatch timestamps                              */
} dmvae_prof_row;
int dmvae_prof_enable(int on);
/* keeps `stream` busy for ~microseconds (<= 20 ms) so the host can run ahead of the GPU and the
 * event brackets of the following launches contain no host launch latency */
int dmvae_debug_spin(void* stream, int microseconds);
int dmvae_prof_collect(dmvae_prof_row* rows, int max_rows);   /* returns number of rows */
/* measurement kernel (csrc/strip_fwd2.hip; tools/strip2_probe.py): Y1 = relu(X . W0 + b0), Y2 = relu(Y1 . W1 + b1), two 512-wide dense layers
 * (base_models.py:220-226) as ONE row-strip launch -- 32 rows per workgroup, Y1 kept in LDS (and written), both weight matrices streamed from L2;
 * bf16 operands, B_pad % 32 == 0, K0 % 64 == 0; same bits as two dmvae_gemm calls with DMVAE_EPI_BIAS_RELU.  Not on the step path. */
int dmvae_debug_strip_fwd2(void* stream, int B_pad, int K0, const void* X, int64_t ldx, const void* W0, int64_t ld0, const float* b0,
                           const void* W1, int64_t ld1, const float* b1, void* Y1, int64_t ldy1, void* Y2, int64_t ldy2);
/* measurement builds only (tools/ablate.sh 6): device pointer of the per-workgroup stamp table of the
 * grouped GEMM kernel, 2048 x {start, end (100 MHz ticks), HW_ID<<32 | XCC_ID, layout<<32 | tile kind};
 * the product library never writes it */
int dmvae_debug_stamps(void** device_ptr);
/* DMVAE_ABLATE=6 builds: per-workgroup phase stamps of the last small-tile bf16 GEMM launch, 2048 x 8 uint64 (100 MHz ticks):
 * {entry, first K tile landed, K loop done, epilogue issued, stores acknowledged, HW_ID << 32 | XCC_ID} (tools/anatomy.py) */
int dmvae_debug_anatomy(void** device_ptr);
/* likewise for the last 256x256 macro-tile launch: 4096 x 8 uint64 {entry, K loop done, epilogue done (100 MHz ticks), HW_ID << 32 | XCC_ID,
 * entry, K loop done (shader cycles, s_memtime), 0, 0} (tools/anatomy256.py; tools/clock256.py: the clock held inside the K loop) */
int dmvae_debug_anatomy256(void** device_ptr);
/* tuning aid: force the bf16 GEMM tile (64|128 x 64|128); (0,0) restores the heuristic */
int dmvae_debug_set_tile(int bm, int bn);
/* tuning aid: knob 0 = supertile height (tile rows) of the L2-friendly tile order,
 *             knob 1 = 8-wave workgroups for the 128-row tiles (0|1),
 *             knob 2 = per-problem tile shapes in the grouped dW grid (0 = all 64x64, 1 = planned, 2 = largest),
 *             (knob 3, the deep-ring policy, was removed in round 4 with its instantiations: measured slower, see csrc/gemm_bf16.hip;
 *              setting it is refused),
 *             knob 4 = XCD runs of a grouped grid cut per tile-shape class (1) or per problem (0),
 *             knob 5 = conv-mode tiles: >= 1 short-K tiles as 4-wave / 2-slot workgroups (three per CU),
 *                      2 also 3-slot rings for the 64x64 weight-gradient tiles,
 *             knob 6 = 256x256 macro-tile kernel (csrc/gemm_bf16_256.hip): 0 never, 1 when its grid covers the chip
 *                      (default), 2 whenever M and N divide by 256,
 *             knob 7 = problems with K <= 128 as 64x64 tiles on a 2-slot ring (32 KiB: four to five workgroups per CU) (0|1;
 *                      default 0: measured slower on the whole step),
 *             knob 8 = merged weight-gradient grid of the 256x256 kernel: first-tile delay, units of 3.4 us spread over the
 *                      256 CUs (default 0 = none, measured best; -1 = one launch per problem),
 *             knob 10 = K slices of the dense weight-gradient group of plans with >= 8192 batch rows (slabs + fixed-order sum in the
 *                      Adam kernel): 0 = the plan's rule (4 where the 256-divisible layers take the macro tile, else 2 from 16384 rows, else none),
 *                      1 = none, 2 | 4 = forced,
 *             knob 11 = with K slices: the 256-divisible layers' slices on the 256x256 macro tile (1, default) or everything on the small tiles (0)
 *             knob 9  = waves per workgroup of a grouped dX launch (0 / 4 = four, 8 = eight at <= 128 VGPRs; tools/heads_dx_probe.py, tools/knob_step.py:
 *                       85.6 vs 90.0 us alone at 16384 rows, 0.9785 vs 0.9651 ms in the step -- four)
 *             knob 12 = the dX of the two head layers as one grouped launch (0 / 1, default) or as two launches (2: 0.9424 vs 0.9366 ms at 16384 rows),
 *             knob 13 = that dX on the streaming kernel (csrc/heads_dx.hip; 1, default, when every problem of the group has K = 64 / 128 / 256) or
 *                       on the grouped tiles (0): the pair alone 20.4 -> 17.4 us at 4096 rows, 80.3 -> 76.8 us at 16384; step -0.6 % at 16384 rows,
 *             knob 14 = blocks the latent kernel's geometry aims at (512; rows per block = 16 .. 64).  The plan sizes its partial sums for the largest
 *                       count and takes the count at enqueue time, so it may change while a plan exists.  1024 at 16384 rows: 0.9500 vs 0.9493 ms,
 *             knob 16 = where the step_finalize blocks run: 1 (default) as riders of the dZ GEMM while tiles + riders <= 256 and its tile has four waves
 *                       (the 64- and 32-row tiles), else as second workgroups of the output layer's dX launch while tiles + riders <= 512 (where they
 *                       also go when a prefetched batch's gather rides in the dZ GEMM), else of the heads' dX launch; 2 always the heads' dX launch;
 *                       3 the output layer's dX launch whenever it has the room, else the heads' dX launch (0.2717 vs 0.2721 ms at 4096 rows);
 *                       0 a launch of their own (0.2796 vs 0.2753 ms at 4096 rows),
 *             knob 17 = where the gather of a prefetched batch (dmvae_plan_prefetch_batch) runs: 1 (default) on the idle CUs of the dZ GEMM, one block
 *                       each, in the last ids of its grid (12.98 us for that launch at 4096 rows, 11.2 without riders); 2 the same in the first ids
 *                       (14.1 us); 3 two blocks per idle CU, last ids (15.5 us); 0 a launch of its own in front of the trunk's backward pass.
 *                       (Those figures: the 64-row dZ tiles of knob 18 = 0.  With the default thin dZ tiles a 4096-row launch is 256 workgroups and has
 *                       no room for riders, so there the gather is a launch of its own whatever this knob says; riders run at <= 2048 rows.)
 *             knob 18 = thin tiles for the dZ GEMM (a 64-wide output with K >= 1024): 2 (default) the thinnest of 16 / 32 rows that still fits one
 *                       round of 256 CUs, 1 down to 32 rows only, 0 the general 64 x 64 tiles (that launch at 4096 rows: 8.92 / 10.19 / 11.49 us),
 *             knob 19 = heads forward + latent stage as ONE launch (csrc/heads_latent.hip) where it applies -- bf16, at most 4096 rows, Dp <= 128, K * D < 4096 -- (1,
 *                       default) or as the grouped heads GEMM + latent_fwd_kernel (0): that pair 26.3 us, the fused launch 25.3 us at 4096 rows; step -0.3 .. -0.8 %,
 *             knob 20 = XCD partition of the grouped weight-gradient launch: runs per tile-shape class by count (0, default) or cut over the whole sequence by streamed
 *                       bytes (1: fetches 13 % less at 8192 rows and is 2 .. 6 % slower on the step at every size: profiles/r05_dw_refetch.txt),
 *             knob 21 = K slices of the thin launches of a small batch (<= 256 rows: the dense layers with K >= 2048 and the dZ GEMM; up to 2048 rows: the fused
 *                       heads + latent launch while blocks x slices <= 256), joined by the last workgroup to arrive (GemmArgs::tick): 1 (default) slices of
 *                       512, 2 slices of 256 (0.1397 vs 0.1402 ms at 100 rows: the same), 0 none,
 *             knob 22 = VaDE's latent stage (dmvae_latent_fwd mode 2) on the large-table form (csrc/latent_vade_mfma.hip) for shapes that fit the
 *                       one-kernel form too (0, default: only where the one-kernel form does not fit; tests/test_gpu_vade_large.py compares the
 *                       two forms).  The caller's dmvae_latent_args.mfma_ws must then hold dmvae_latent_vade_ws_bytes(.., forced = 1, ..) bytes:
 *                       without them the call is DMVAE_EINVAL, it never falls back to the one-kernel form.  Plans reserve that scratch (and size
 *                       their prior-gradient partials) by the shape alone, so while the knob is set the steps of a plan whose shape fits the
 *                       one-kernel form fail with that DMVAE_EINVAL: the knob is for callers of dmvae_latent_fwd. */
int dmvae_debug_set_knob(int which, int value);

/* ---- the CNN trunk's kernels on caller-owned buffers (csrc/conv.hip; tests/test_gpu_conv_kernels.py) ----------
 * dtype = DMVAE_F32 | DMVAE_BF16 is the activation AND weight type.  A zero-bordered activation is [n_img][P][P][ld], P = side + 2,
 * and pointers to one address padded pixel 0; the conv-mode GEMMs read up to P + 1 rows in front of it and behind its end.
 * first layer: x = [n_img][bstride] images of H x H pixels (H % 4 == 0), W = [9][ldw] with 32 outputs, out / dY = [n_img][H+2][H+2][ld], ld = 32 | 64;
 * the forward writes interior pixels only. */
int dmvae_debug_conv_first_fwd(void* stream, int dtype, const void* x, int64_t bstride, int H, int64_t n_img, const void* W, int ldw,
                               const float* bias, void* out, int ld);
/* dW = [9][ldw], db = [32]; *n_blocks = the partial-sum blocks of this geometry; part = n_blocks x 320 floats of scratch (part == NULL: only the count) */
int dmvae_debug_conv_first_dw(void* stream, int dtype, const void* x, int64_t bstride, int H, int64_t n_img, const void* dY, int ld,
                              float* dW, int ldw, float* db, float* part, int64_t part_floats, int* n_blocks);
int dmvae_debug_zero_border(void* stream, int dtype, void* a, int P, int ld, int64_t n_img);
/* SAME 2x2 / stride-2 max-pool of a zero-bordered [n_img][H+2][H+2][ld]; out is zero-bordered (out_border = 1: interior written only) or plain */
int dmvae_debug_maxpool2_fwd(void* stream, int dtype, const void* in, int H, int ld, int64_t n_img, void* out, int out_border);
/* its gradient behind a ReLU: first maximum of the window in row-major order, gated by in > 0; writes the interior pixels of din */
int dmvae_debug_maxpool2_bwd_relu(void* stream, int dtype, const void* in, const void* dout, int H, int ld, int64_t n_img, void* din, int dout_border);
/* W = [9 * cin][ldw] -> Wt = [cin_ld][Kt], column (tap, co) = W[(8 - tap, ci)][co]; zero pad rows / columns */
int dmvae_debug_conv_wflip(void* stream, int dtype, const void* W, int cin, int cin_ld, int cout, int ldw, void* Wt, int Kt);
/* dmvae_gemm in conv mode (implicit 3x3 SAME convolution over padded pixel rows): conv_p = P, conv_c = channels per tap of the A operand;
 * FWD + BIAS_RELU, DX + RELU_MASK, DW + ATOMIC_F32 / STORE_F32; epi->n_valid = the real output columns */
int dmvae_debug_conv_gemm(void* stream, int dtype, int layout, int M, int N, int K, const void* A, int64_t lda,
                          const void* B, int64_t ldb, const dmvae_epilogue* epi, int split_k, int conv_p, int conv_c);
/* weight + bias gradient of one convolution layer exactly as the plan's backward pass runs it, for a given K split over `rows` padded pixel rows:
 * dW = [pad64(9 * conv_c)][N], db = [N] (both zeroed first); split 1: fp32 atomics; split > 1: K-slice slabs in `slab`
 * (split * (pad64(9 * conv_c) + 1) * N floats) added in a fixed order; the pad rows past the ninth tap are zeroed */
int dmvae_debug_conv_dw(void* stream, int dtype, int rows, int conv_p, int conv_c, const void* X, int64_t ldx, const void* dY, int64_t ldy,
                        int N, int n_valid, int split, float* slab, float* dW, float* db);

/* ---- step_finalize and the rider launches on caller-owned buffers (csrc/common.h step_finalize_block, csrc/gemm_epilogue.h gather_rows_block;
 * tests/test_gpu_step_finalize.py) ----------
 * step_finalize_block is compiled into five kernels: its own, the dense dX GEMM that carries riders (LATENT = the dZ GEMM, RELU_MASK = a layer's dX),
 * the grouped dX tiles and the streaming dX of the head layers; gather_rows_block into its own kernel and the dense dX GEMM.  The step picks the home
 * by shape and knobs (csrc/step.hip place_riders); these entries reach every home on buffers of the caller's.
 * rp = nr reconstruction-loss partials, lp = nl pairs {kl_z, kl_c}, state = a dmvae_state on the device (read and written), part = [nblk][ncol] prior-table
 * gradient partials -> gout[ncol]; bump_adam: advance adam_t and write lr_t (b1, b2). */
typedef struct dmvae_debug_finalize {
    const float* rp; int nr;
    const float* lp; int nl;
    float inv_B; void* state; int bump_adam;
    float b1, b2;
    const float* part; int nblk, ncol;
    float* gout;
} dmvae_debug_finalize;
/* the arguments of dmvae_gather_rows with a bf16 output only: out_bf16 = [B_pad][ld], every column written (pad rows and columns: zeros) */
typedef struct dmvae_debug_gather {
    const float* data; int64_t n_rows; int dim;
    const int32_t* perm; int64_t first;
    int batch, n_valid, B_pad;
    void* out_bf16; int64_t ld;
    const void* state;
} dmvae_debug_gather;
/* the stand-alone kernel (1 + ceil(ncol / 16) workgroups) */
int dmvae_debug_step_finalize(void* stream, const dmvae_debug_finalize* fin);
/* dmvae_gemm(bf16, DMVAE_GEMM_DX, LATENT | RELU_MASK epilogue, no K split) with riders in its grid: the step_finalize blocks in the first
 * (nblocks + 7) & ~7 ids (fin, may be NULL) and / or ngat workgroups of the gather (gat, may be NULL; ngat a multiple of 8) behind them, or --
 * gat_last -- in the last ids of the grid.  DMVAE_EINVAL: ngat not a multiple of 8; a launch without the room (small dense tiles only, tiles + riders
 * <= 512); fin on the two-wave 16-row tile of the dZ GEMM; fin together with a gather addressed through the state's batch cursor (finalize advances
 * the cursor the gather reads: the step never puts the two into one launch). */
int dmvae_debug_gemm_dx_riders(void* stream, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, const dmvae_epilogue* epi,
                               const dmvae_debug_finalize* fin, const dmvae_debug_gather* gat, int ngat, int gat_last);
/* dmvae_gemm_grouped(bf16, DMVAE_GEMM_DX) of RELU_MASK problems with the step_finalize blocks riding: on the streaming kernel where it takes the group
 * (csrc/heads_dx.hip, knob 13), else on the grouped tiles */
int dmvae_debug_gemm_grouped_fin(void* stream, const dmvae_gemm_problem* probs, int n, const dmvae_debug_finalize* fin);

/* ---- the 256x256 macro tile with the arguments only the step sets (csrc/gemm_bf16_256.hip; tests/test_gpu_gemm256_forms.py) ----------
 * bf16 problems sent to the macro tile whatever knob 6 says, each with
 *   csum_out  FWD + BIAS_RECON / DX + RELU_MASK: the column sums of the bf16-rounded output per 256-row tile -> [M / 256][csum_ld] (NULL: none),
 *   csum_in   DW with a bias gradient (epi.out2): such partials, [csum_rows][csum_ld] with csum_ld = N; db = their ascending sum (and its Adam
 *             update) in the launch's extra workgroups, instead of the slab column sums of B (NULL: those),
 *   k_split   DW + STORE_F32: K slices of this depth (a multiple of 64 that divides K), slice y -> out + y * slab_stride; 0 or K: no slices.
 * FWD / DX: n = 1 -> gemm_bf16_256_launch; DW: n problems -> gemm_bf16_256_dw_all (merged into one grid where possible), ctx for DMVAE_EPI_ADAM.
 * Validates like dmvae_gemm; DMVAE_EUNSUPPORTED for a (layout, epilogue) pair the macro tile is not instantiated for, DMVAE_EINVAL for a shape
 * that does not divide by 256 x 256 x 64 and for arguments the launchers refuse (K slices with ADAM, with epi.out2 or without slab_stride;
 * csum_ld != N on csum_in). */
typedef struct dmvae_debug_gemm256_problem {
    dmvae_gemm_problem p;
    float* csum_out;
    const float* csum_in;
    int64_t csum_ld;
    int csum_rows, k_split;
    int64_t slab_stride;
} dmvae_debug_gemm256_problem;
int dmvae_debug_gemm256(void* stream, int layout, const dmvae_debug_gemm256_problem* probs, int n, const dmvae_adam_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DMVAE_HIP_DEBUG_H */
