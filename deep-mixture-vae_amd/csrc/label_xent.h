// Arguments of the semi-supervised label stage (label_xent.hip), shared by the kernel, the stand-alone entry dmvae_label_xent (api.hip)
// and the step plan (step.hip: label_stage).
#pragma once
#include "common.h"

namespace dmvae {

constexpr int LABEL_ROWS_PER_BLOCK = 4;      // one 64-lane wave per row
constexpr int LABEL_ACC_HEAD = 8;            // doubles in front of the scratch: six results, the top ticket, one spare
constexpr int LABEL_GROUP = 64;              // workgroups that share one group ticket
constexpr int LABEL_GROUP_STRIDE = 16;       // doubles per group ticket: a 128-byte line each
constexpr int LABEL_ERR_CLASS = 1;           // a label outside {-1} u [0, K)
constexpr int LABEL_ERR_PERM = 2;            // a permutation entry (or first + r) outside [0, label_rows)

struct LabelXentArgs {
    const float* logits; int64_t ld_lg;  // [n_valid][>= K] f32
    int32_t n_valid, K;
    const int32_t* labels; int64_t label_rows;       // [label_rows] int32 in data-set row order, -1 = unlabelled
    const int32_t* perm; int64_t first;  // batch row r is data-set row perm[first + r] (perm null: first + r)
    int32_t batch, act_dtype;
    const dmvae_state* st;               // non-null: first = st->batch_cursor * batch
    float scale;                         // the host's share of the coefficient (the plan: inv_B)
    const float* w;                      // the device's share (the plan: "label_ctl"[0]); null: 1
    void* dlogits; int64_t ld_dl;        // [n_valid][>= K] act dtype: += w * scale * (q - onehot) in labelled rows, nothing else is written
    float* row_loss;                     // optional [n_valid]: l_r, 0 in rows without a label
    double* acc;                         // [label_xent_acc_elems(n_valid)], see dmvae_hip.h
    int32_t* err_flag;
};

int label_xent_nblocks(int n_valid);
int64_t label_xent_acc_elems(int n_valid);
int label_xent_launch(hipStream_t s, const LabelXentArgs& a, const char* who);

}  // namespace dmvae
