// Arguments of the mixture-of-experts row stage (moe_head.hip), shared by the kernel and the step plan (step.hip: moe_stage).
#pragma once
#include "common.h"

namespace dmvae {

struct MoeHeadArgs {
    int32_t B, B_pad;                   // rows that are real; rows [B, B_pad) write zeros
    int32_t E, O;                       // experts (= the gate's clusters), outputs
    int32_t featLearn, classification, backward, act_dtype;
    float inv_B;                        // 1 / n_valid: scale of every gradient and of the batch loss
    float* P; int64_t ldP;              // [B_pad][>= E*O] f32 expert outputs, column e*O + o; featLearn: written here.  backward: dP (f32) on return
    const float* logits; int64_t ld_lg; // [B_pad][>= E]
    const float* Y; int64_t n_rows;     // labels [n_rows][O] f32 (the dataset's, resident)
    const int32_t* perm; int64_t first; int32_t batch, reserved;
    const dmvae_state* st;              // non-null: first = st->batch_cursor * batch
    // featLearn (inp = relu(mean)): the expert weights [D][ldW] (f32 master, column e*O + o) and bias [E*O]
    const float* mean; int64_t ld_mean; int32_t D, Dp;
    const float* W; int64_t ldW; const float* bias;
    void* inp_act; int64_t ld_inp;      // [B_pad][Dp] act: relu(mean), the weight-gradient operand
    float* gmu; int64_t ld_g;           // += d(relu input) * [mean > 0]
    void* dP_act; int64_t ld_dP;        // [B_pad][ld_dP] act: dP, the weight-gradient operand
    void* dlogits_act; int64_t ld_dl;   // += q (dq - sum q dq)
    float* dq_ws; int64_t ld_dq;        // [B_pad][>= E] scratch
    float* pred; int64_t ld_pred;       // optional [B_pad][O]: reconstructed_Y_soft (classification) / reconstructed_Y (regression)
    float* partials;                    // [moe_head_nblocks][2]
    float* acc;                         // [4]: epoch loss_moe, epoch error, batch loss_moe, batch error
};

int moe_head_nblocks(int B_pad);
int moe_head_launch(hipStream_t s, const MoeHeadArgs& a);

}  // namespace dmvae
