"""The host-side layout of a step plan, as plain data: dmvae_sizes, the tensor table, dmvae_plan_grad_buckets and every view
dmvae_plan_view knows (offset from the workspace base, ld, dtype -- or the error).  Host only: the plan is bound to made-up
256-aligned addresses and nothing is dereferenced.

    python tests/helpers/plan_layout_dump.py        rewrites tests/golden/plan_layout.json

tests/test_plan_layout_golden.py compares collect() against that file exactly.  The file is regenerated only by a change that
moves a buffer on purpose."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))
from dmvae_hip import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_layout.json")
F32, BF16 = _lib.F32, _lib.BF16
MNIST = dict(I=784, enc=(500, 500), head=2000, dec=(2000, 500, 500))

CONFIGS = [
    # the eight geometries of tests/helpers/asan_plan_probe.py
    dict(name="cfg1_f32_100", D=10, K=10, B=100, dt=F32, **MNIST),
    dict(name="cfg2_bf16_4096", D=64, K=10, B=4096, dt=BF16, **MNIST),
    dict(name="cfg3_bf16_16384", D=128, K=10, B=16384, dt=BF16, **MNIST),
    dict(name="cfg4_bf16_8192", D=256, K=50, B=8192, dt=BF16, **MNIST),
    dict(name="cfg5_bf16_8192", I=4096, D=512, K=256, enc=(4096,) * 4, head=4096, dec=(4096,) * 4, B=8192, dt=BF16),
    dict(name="cnn_bf16_256", I=784, D=64, K=10, enc=(500,), head=2000, dec=(2000, 500, 500), B=256, dt=BF16, trunk=1),
    dict(name="deep_f32_37", I=96, D=8, K=4, enc=(64,) * 8, head=64, dec=(64,) * 8, B=37, dt=F32),
    dict(name="vade_cnn_bf16_128", I=784, D=10, K=10, enc=(128,), head=64, dec=(500, 500, 2000), B=128, dt=BF16, trunk=1, model=1),
    # the step's small batch in bf16 (K-slice scratch), VaDE off the MLP trunk (small and large prior tables), MoE attachments
    dict(name="cfg1_bf16_100", D=10, K=10, B=100, dt=BF16, **MNIST),
    dict(name="vade_mlp_bf16_128", I=784, D=10, K=10, enc=(500, 500, 2000), head=64, dec=(2000, 500, 500), B=128, dt=BF16, model=1),
    dict(name="vade_large_bf16_128", I=784, D=256, K=50, enc=(500, 500, 2000), head=64, dec=(2000, 500, 500), B=128, dt=BF16, model=1),
    dict(name="cfg2_bf16_256_moe", D=64, K=10, B=256, dt=BF16, moe=dict(E=10, O=10, featLearn=0), **MNIST),
    dict(name="cfg2_bf16_256_moe_featlearn", D=64, K=10, B=256, dt=BF16, moe=dict(E=10, O=10, featLearn=1), **MNIST),
]

VIEWS = (["mean", "log_var", "logits", "weights", "eval_w", "recon", "x", "Z", "dxlogits", "moe_P", "moe_pred", "moe_acc", "hzc", "flat"]
         + ["enc%d" % i for i in range(8)] + ["dec%d" % i for i in range(8)] + ["conv%d" % i for i in range(6)])

# made-up device addresses, 256-byte aligned and far apart
FAKE = dict(param=0x100000000000, grad=0x200000000000, m=0x300000000000, v=0x400000000000, param_bf16=0x500000000000,
            work=0x600000000000, state=0x700000000000, labels=0x710000000000)


def make_config(c):
    cfg = _lib.Config()
    cfg.input_dim, cfg.latent_dim, cfg.n_classes = c["I"], c["D"], c["K"]
    cfg.n_enc, cfg.head_dim, cfg.n_dec = len(c["enc"]), c["head"], len(c["dec"])
    for i, v in enumerate(c["enc"]):
        cfg.enc[i] = v
    for i, v in enumerate(c["dec"]):
        cfg.dec[i] = v
    cfg.dtype, cfg.max_batch, cfg.trunk, cfg.model = c["dt"], c["B"], c.get("trunk", 0), c.get("model", 0)
    cfg.temperature, cfg.beta1, cfg.beta2, cfg.adam_eps = 1.0, 0.9, 0.999, 1e-8
    return cfg


def layout_of(c):
    lib = _lib.lib
    cfg = make_config(c)
    h = C.c_void_p()
    _lib.check(lib.dmvae_plan_create(C.byref(cfg), C.byref(h)), "dmvae_plan_create")
    try:
        if c.get("moe"):
            mc = _lib.MoeConfig()
            mc.n_experts, mc.output_dim, mc.featLearn = c["moe"]["E"], c["moe"]["O"], c["moe"]["featLearn"]
            mc.classification, mc.lossVAE, mc.labels, mc.label_rows = 1, 1, FAKE["labels"], 1024
            _lib.check(lib.dmvae_plan_attach_moe(h, C.byref(mc)), "dmvae_plan_attach_moe")
        sz = _lib.Sizes()
        _lib.check(lib.dmvae_plan_sizes(h, C.byref(sz)), "dmvae_plan_sizes")
        out = dict(sizes=dict(param_elems=sz.param_elems, work_bytes=sz.work_bytes, batch_pad=sz.batch_pad, input_pad=sz.input_pad,
                              n_tensors=sz.n_tensors))
        out["tensors"] = []
        for i in range(sz.n_tensors):
            ti = _lib.TensorInfo()
            _lib.check(lib.dmvae_plan_tensor(h, i, C.byref(ti)), "dmvae_plan_tensor")
            out["tensors"].append([ti.name.decode(), ti.offset, ti.rows, ti.cols, ti.ld])
        b = (C.c_int64 * 5)()
        _lib.check(lib.dmvae_plan_grad_buckets(h, b), "dmvae_plan_grad_buckets")
        out["grad_buckets"] = list(b)
        bufs = _lib.Buffers(FAKE["param"], FAKE["grad"], FAKE["m"], FAKE["v"], FAKE["param_bf16"], FAKE["work"], FAKE["state"], 0)
        _lib.check(lib.dmvae_plan_bind(h, C.byref(bufs)), "dmvae_plan_bind")
        out["views"] = {}
        for name in VIEWS:
            p, ld, dt = C.c_void_p(), C.c_int64(), C.c_int32()
            rc = lib.dmvae_plan_view(h, name.encode(), C.byref(p), C.byref(ld), C.byref(dt))
            if rc:
                out["views"][name] = dict(error=rc, message=lib.dmvae_last_error().decode())
            else:
                out["views"][name] = dict(offset=p.value - FAKE["work"], ld=ld.value, dtype=dt.value)
        return out
    finally:
        lib.dmvae_plan_destroy(h)


def collect():
    return {c["name"]: layout_of(c) for c in CONFIGS}


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(collect(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % GOLDEN)
