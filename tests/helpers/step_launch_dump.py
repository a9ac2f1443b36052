"""What the library enqueues for one eager pass, per case: the rows of dmvae_prof_collect (name, launches, kernel_launches, flops,
bytes; no times) after every operation of the case, in order.  The cases are the smallest shapes at which each branch of the
step's orchestration is taken (K slices of thin launches, the fused heads + latent launch, step_finalize riding or alone, gather
riders, the macro tile's column-sum hand-over, the staged backward, VaDE's two latent forms, the CNN trunk, the MoE stage, the
sliced dW group with slabs / bias strips / adam_slabs / slab_reduce) plus the evaluators that share the plan's buffers.

    python tests/helpers/step_launch_dump.py        (on the GPU) rewrites tests/golden/step_launches.json

tests/test_gpu_step_launches.py compares run_case() against that file exactly.  A change that alters the launch structure on
purpose regenerates the file and shows the diff; nothing else does."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_launches.json")
KNOB_DEFAULTS = {6: 1, 10: 0, 11: 1}

CFG1 = dict(input_dim=784, latent_dim=10, n_classes=10)
MACRO = dict(input_dim=256, latent_dim=64, n_classes=10, enc_layers=(256, 256), head_dim=256, dec_layers=(256, 256))
SLABS = dict(input_dim=64, latent_dim=64, n_classes=10, enc_layers=(256,), head_dim=128, dec_layers=(256,))
VADE = dict(input_dim=784, n_classes=10, model="vade", head_dim=64, enc_layers=(500, 500, 2000), dec_layers=(2000, 500, 500))
MOE = dict(input_dim=784, latent_dim=64, n_classes=10)

CASES = [
    dict(name="cfg1_bf16_100", B=100, dtype="bf16", kw=CFG1, ops=("fb", "step", "eval")),
    dict(name="cfg1_f32_100", B=100, dtype="fp32", kw=CFG1, ops=("fb", "step", "eval")),
    dict(name="cfg1_bf16_100_prefetch", B=100, dtype="bf16", kw=CFG1, ops=("pipelined",)),
    dict(name="macro_bf16_256", B=256, dtype="bf16", kw=MACRO, knobs={6: 2}, ops=("fb", "step")),
    dict(name="cfg1_bf16_100_stages3", B=100, dtype="bf16", kw=CFG1, ops=("stages3",)),
    dict(name="cfg1_bf16_100_stages2", B=100, dtype="bf16", kw=CFG1, ops=("stages2",)),
    dict(name="cfg1_f32_100_stages3", B=100, dtype="fp32", kw=CFG1, ops=("stages3",)),
    dict(name="vade_bf16_128", B=128, dtype="bf16", kw=dict(VADE, latent_dim=10), ops=("fb", "step", "stages3", "eval")),
    dict(name="vade_large_bf16_128", B=128, dtype="bf16", kw=dict(VADE, latent_dim=256, n_classes=50), ops=("fb", "step", "eval")),
    dict(name="cnn_bf16_128", B=128, dtype="bf16", kw=dict(CFG1, enc_layers=(500,), cnn=True), ops=("fb", "step")),
    dict(name="cnn_f32_128", B=128, dtype="fp32", kw=dict(CFG1, enc_layers=(500,), cnn=True), ops=("fb",)),
    dict(name="moe_bf16_128", B=128, dtype="bf16", kw=MOE, moe=0, ops=("fb", "step", "moe_predict")),
    dict(name="moe_featlearn_bf16_128", B=128, dtype="bf16", kw=MOE, moe=1, ops=("fb", "step", "moe_predict")),
] + [
    dict(name="slabs_bf16_8192_k10_%d_k11_%d" % (s, m), B=8192, dtype="bf16", kw=SLABS, knobs={10: s, 11: m}, ops=("step", "fb_only"))
    for s in (2, 4) for m in (0, 1)
]


def make_engine(case, seed=0):
    """(engine, data, perm) of a case: parameters from `seed`, a data set of two batches"""
    from dmvae_hip import StepEngine
    B, kw = case["B"], dict(case["kw"])
    g = torch.Generator().manual_seed(1234)
    X = (torch.rand(2 * B, kw["input_dim"], generator=g) > 0.5).float().cuda()
    perm = torch.randperm(2 * B, generator=g).to(torch.int32).cuda()
    if "moe" in case:
        labels = torch.nn.functional.one_hot(torch.randint(0, 10, (2 * B,), generator=g), 10).float().cuda()
        kw["moe"] = dict(n_experts=10, output_dim=10, featLearn=case["moe"], classification=True, lossVAE=True, labels=labels)
    eng = StepEngine(dtype=case["dtype"], max_batch=B, seed=77, **kw)
    eng.init_parameters(seed)
    eng.reset_epoch(2)
    return eng, X, perm


def run_op(eng, op, X, perm):
    from dmvae_hip import _lib
    B = eng.max_batch
    if op == "fb":
        eng.load_batch(X, perm, 0, B)
        eng.forward_backward(B)
        eng.update(1.0)
    elif op == "fb_only":
        eng.load_batch(X, perm, 0, B)
        eng.forward_backward(B)
    elif op == "step":
        eng.train_step(X, perm, B)
    elif op == "pipelined":      # two steps, each assembling the next batch under its own backward pass
        eng._load_batch_for_step(X, perm, 0, None, True)
        for _ in range(2):
            eng._prefetch_batch(X, perm)
            eng.forward_backward_update(B)
            _lib.check(_lib.lib.dmvae_plan_swap_batch(eng._plan), "dmvae_plan_swap_batch")
    elif op in ("stages3", "stages2"):
        eng.set_stage_groups(int(op[-1]))
        eng.load_batch(X, perm, 0, B)
        for stage in (0, 1, 2):
            eng.forward_backward_stage(stage, B)
        eng.set_stage_groups(3)
    elif op == "eval":
        classes = torch.zeros(X.shape[0], dtype=torch.int32, device="cuda")
        conf, acc = eng.confusion_buffer(eng.n_classes, "cuda"), eng.loglik_buffer()
        eng.load_batch(X, None, 0, B)
        eng.encode(B)
        eng.eval_clusters(conf, classes, None, 0, B, draws=2, counter=3)
        eng.eval_loglik(acc, B, X.shape[0], 0, 2, counter=5)
        eng.decode(torch.zeros(B, eng.latent_dim, device="cuda"))
    elif op == "moe_predict":
        eng.load_batch(X, perm, 0, B)
        eng.moe_predict(B)
    else:
        raise ValueError(op)


def run_case(case):
    """[[op, [[name, launches, kernel_launches, flops, bytes], ...]], ...] of one case"""
    from dmvae_hip import _lib, runtime
    out = []
    try:
        for k, v in case.get("knobs", {}).items():
            _lib.check(_lib.lib.dmvae_debug_set_knob(k, v), "knob")
        eng, X, perm = make_engine(case)
        torch.cuda.synchronize()
        runtime.prof_enable(True)
        for op in case["ops"]:
            run_op(eng, op, X, perm)
            torch.cuda.synchronize()
            out.append([op, [[r["name"], r["launches"], r["kernel_launches"], r["flops"], r["bytes"]] for r in runtime.prof_collect(256)]])
    finally:
        runtime.prof_enable(False)
        runtime.prof_collect(256)
        for k, v in KNOB_DEFAULTS.items():
            _lib.lib.dmvae_debug_set_knob(k, v)
    return out


if __name__ == "__main__":
    torch.cuda.set_device(0)
    res = {c["name"]: run_case(c) for c in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d launches" % (GOLDEN, len(res), sum(r[1] for ops in res.values() for _, rows in ops for r in rows)))
