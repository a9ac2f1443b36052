// Semi-supervised DMVAE: cross-entropy on q(c|x) = softmax(logits) for the batch rows that carry a label.  The stage runs behind the latent
// stage of a step whose plan carries a label attachment (dmvae_plan_attach_labels) and is the whole of dmvae_label_xent.
//
//   i_r = perm[first + r]                  (first = state->batch_cursor * batch with the device cursor: the addressing of moe_head.hip)
//   y_r = labels[i_r]                      (-1: no label -- the row is left alone)
//   l_r = logsumexp(logits_r) - logits_r[y_r]
//   dlogits_r[k] += w * scale * (q_r[k] - [k == y_r])      q_r = softmax(logits_r), f32, the maximum subtracted; act dtype: f32 add, then
//                                                          round to nearest even
// Nothing else of dlogits is written: rows without a label, rows >= n_valid and columns >= K keep their bits, and so does every row while
// w * scale == 0 (a sum with +0 would turn a -0 into +0).  A label outside {-1} u [0, K) or a row index outside [0, label_rows) sets a bit
// of the error flag and the row is skipped.
//
// Layout: one 64-lane wave per row, four waves per workgroup.  The wave fetches its label first; without one it goes straight to the
// workgroup's join (with 100 labels in 70 000 rows almost every wave does only that).  Lanes stride over K (any K: the wave loops); the
// arg-max, the maximum and the sum of exponentials are butterfly reductions over the 64 lanes, which leave the same bits in every lane.
// Loss and counts: one partial triple per workgroup that holds a labelled row (rows in ascending order), tickets (integer atomics), and
// the last workgroup to arrive adds the partials in ascending order in float64 -- no float atomics, two runs give the same bits.  The
// counts are float64 too: exact to 2^53.
#include "label_xent.h"

namespace dmvae {

constexpr int LX_ROWS = LABEL_ROWS_PER_BLOCK;

__device__ __forceinline__ void lx_store(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double lx_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__global__ __launch_bounds__(64 * LX_ROWS) void label_xent_kernel(LabelXentArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * LX_ROWS + wv;
    const int K = a.K;

    // the row's label through the batch permutation (wave-uniform)
    int y = -1;
    if (r < a.n_valid) {
        const int64_t first = a.st ? (int64_t)a.st->batch_cursor * a.batch : a.first;
        const int64_t i = first + r;
        const int64_t src = a.perm ? (int64_t)a.perm[i] : i;
        if (src < 0 || src >= a.label_rows) {
            if (lane == 0) atomicOr(a.err_flag, LABEL_ERR_PERM);
        } else {
            y = a.labels[src];
            if (y < -1 || y >= K) {
                if (lane == 0) atomicOr(a.err_flag, LABEL_ERR_CLASS);
                y = -1;
            }
        }
    }

    float loss = 0.f;
    int correct = 0;
    if (y >= 0) {
        const float* lg = a.logits + (int64_t)r * a.ld_lg;
        // arg-max (np.argmax's rule: the first index of the largest) and with it the maximum
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int k = lane; k < K; k += 64) {
            const float v = lg[k];
            if (v > bv) { bv = v; bi = k; }       // ascending k within the lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        const float mx = bv;
        float se = 0.f;
        for (int k = lane; k < K; k += 64) se += expf(lg[k] - mx);
        se = wave_sum(se);
        loss = logf(se) + (mx - lg[y]);
        correct = bi == y;
        const float c = (a.w ? *a.w : 1.f) * a.scale;
        if (c != 0.f) {
            const float inv = 1.f / se;
            for (int k = lane; k < K; k += 64) {
                const float d = c * (expf(lg[k] - mx) * inv - (k == y ? 1.f : 0.f));
                const int64_t i = (int64_t)r * a.ld_dl + k;
                if (a.act_dtype == DMVAE_BF16) {
                    bf16_t* dl = reinterpret_cast<bf16_t*>(a.dlogits);
                    dl[i] = f2bf(bf2f(dl[i]) + d);
                } else {
                    float* dl = reinterpret_cast<float*>(a.dlogits);
                    dl[i] = dl[i] + d;
                }
            }
        }
    }
    if (a.row_loss && r < a.n_valid && lane == 0) a.row_loss[r] = loss;

    // the workgroup's partial: rows in ascending order
    __shared__ float s_loss[LX_ROWS];
    __shared__ int s_n[LX_ROWS], s_ok[LX_ROWS], s_last;
    __shared__ double red[64 * LX_ROWS][3];
    if (lane == 0) { s_loss[wv] = loss; s_n[wv] = y >= 0; s_ok[wv] = correct; }
    __syncthreads();
    // Scratch behind the results (LABEL_ACC_HEAD): one ticket per group of LABEL_GROUP workgroups, each on a 128-byte line of its own, then
    // one partial triple per workgroup.  Everything there is ZERO between launches: a workgroup without a labelled row stores nothing
    // and only takes its group's ticket (a relaxed add); the last of a group takes the top ticket; the last of all adds up the slots
    // in ascending order and clears the ones it found written.  Same-address atomics: at most LABEL_GROUP per group ticket, one per group on
    // the top one (a single ticket for all 1024 workgroups of a 4096-row batch made the launch 27 us).
    const int nblk = gridDim.x, ngrp = (nblk + LABEL_GROUP - 1) / LABEL_GROUP;
    unsigned int* tick = reinterpret_cast<unsigned int*>(a.acc + 6);
    double* part = a.acc + LABEL_ACC_HEAD + (int64_t)LABEL_GROUP_STRIDE * ngrp;
    if (threadIdx.x == 0) {
        double l = 0.0;
        int n = 0, ok = 0;
#pragma unroll
        for (int j = 0; j < LX_ROWS; ++j) { l += (double)s_loss[j]; n += s_n[j]; ok += s_ok[j]; }
        const int g = blockIdx.x / LABEL_GROUP;
        const int gsize = min(LABEL_GROUP, nblk - g * LABEL_GROUP);
        unsigned int* gtick = reinterpret_cast<unsigned int*>(a.acc + LABEL_ACC_HEAD + (int64_t)LABEL_GROUP_STRIDE * g);
        unsigned int t;
        if (n > 0) {
            lx_store(part + 3 * (int64_t)blockIdx.x, l);
            lx_store(part + 3 * (int64_t)blockIdx.x + 1, (double)n);
            lx_store(part + 3 * (int64_t)blockIdx.x + 2, (double)ok);
            t = __hip_atomic_fetch_add(gtick, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);       // the partial is visible before the ticket
        } else {
            t = __hip_atomic_fetch_add(gtick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        bool last = false;
        if (t == (unsigned int)(gsize - 1)) {
            // the group's last: what the group published goes on with the top ticket (acquire from the group's, release into the top one)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(gtick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = __hip_atomic_fetch_add(tick, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned int)(ngrp - 1);
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double l = 0.0, n = 0.0, ok = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64 * LX_ROWS) {
        const double pl = lx_load(part + 3 * (int64_t)i), pn = lx_load(part + 3 * (int64_t)i + 1), pk = lx_load(part + 3 * (int64_t)i + 2);
        l += pl; n += pn; ok += pk;
        if (pn != 0.0) {                             // a written slot (a labelled row at least): back to zero for the next launch
            lx_store(part + 3 * (int64_t)i, 0.0); lx_store(part + 3 * (int64_t)i + 1, 0.0); lx_store(part + 3 * (int64_t)i + 2, 0.0);
        }
    }
    red[threadIdx.x][0] = l; red[threadIdx.x][1] = n; red[threadIdx.x][2] = ok;
    __syncthreads();
    for (int s = 32 * LX_ROWS; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int j = 0; j < 3; ++j) red[threadIdx.x][j] += red[threadIdx.x + s][j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { a.acc[j] += red[0][j]; a.acc[3 + j] = red[0][j]; }
        __hip_atomic_store(tick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next launch starts from zero
    }
}

int label_xent_nblocks(int n_valid) { return (n_valid + LX_ROWS - 1) / LX_ROWS; }
int64_t label_xent_acc_elems(int n_valid) {
    const int64_t nblk = label_xent_nblocks(n_valid > 0 ? n_valid : 0);
    return LABEL_ACC_HEAD + LABEL_GROUP_STRIDE * ((nblk + LABEL_GROUP - 1) / LABEL_GROUP) + 3 * nblk;
}

#define LX_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int label_xent_launch(hipStream_t s, const LabelXentArgs& a, const char* who) {
    LX_REQUIRE(a.logits, "%s: null logits", who);
    LX_REQUIRE(a.labels, "%s: null labels", who);
    LX_REQUIRE(a.dlogits, "%s: null dlogits", who);
    LX_REQUIRE(a.acc, "%s: null acc", who);
    LX_REQUIRE(a.err_flag, "%s: null err_flag", who);
    LX_REQUIRE(a.K >= 1, "%s: K=%d (>= 1)", who, a.K);
    LX_REQUIRE(a.n_valid >= 0, "%s: n_valid=%d (>= 0)", who, a.n_valid);
    LX_REQUIRE(a.ld_lg >= a.K, "%s: ld_lg=%lld < K=%d", who, (long long)a.ld_lg, a.K);
    LX_REQUIRE(a.ld_dl >= a.K, "%s: ld_dl=%lld < K=%d", who, (long long)a.ld_dl, a.K);
    LX_REQUIRE(a.label_rows >= 1, "%s: label_rows=%lld (>= 1)", who, (long long)a.label_rows);
    LX_REQUIRE(a.act_dtype == DMVAE_F32 || a.act_dtype == DMVAE_BF16, "%s: act_dtype=%d (DMVAE_F32 or DMVAE_BF16)", who, a.act_dtype);
    LX_REQUIRE(a.scale == a.scale && a.scale - a.scale == 0.f, "%s: scale is not finite", who);
    if (!a.st) {
        LX_REQUIRE(a.first >= 0, "%s: first=%lld (>= 0)", who, (long long)a.first);
        LX_REQUIRE(a.perm || a.first + a.n_valid <= a.label_rows, "%s: without perm, rows [first=%lld, +n_valid=%d) must lie inside label_rows=%lld", who,
                   (long long)a.first, a.n_valid, (long long)a.label_rows);
    }
    if (a.n_valid == 0) return 0;
    // (as if every row were labelled: the logits three times, dlogits read and written, label and permutation entry)
    ProfScope ps(s, "label_xent", 8.0 * a.n_valid * a.K, (double)a.n_valid * ((12.0 + 2.0 * (a.act_dtype == DMVAE_BF16 ? 2 : 4)) * a.K + 8.0));
    DMVAE_LAUNCH(label_xent_kernel, dim3(label_xent_nblocks(a.n_valid)), dim3(64 * LX_ROWS), 0, s, a);
    return check_launch("label_xent");
}

}  // namespace dmvae
