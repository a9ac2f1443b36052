"""Shared by tests/test_moe_host.py and tests/test_gpu_moe_head.py: the cases of the mixture-of-experts row stage (csrc/moe_head.hip), the float64
oracle and the float32 yardstick (moe_oracle.head_f32) on a set of head inputs, and the tolerance rule.

A case is a whole parameter set of the small MLP stack (SMALL), a data set X, labels Y and a fixed batch order; get_case builds it on the CPU from
the float64 encoder of oracle/dmvae_oracle.py, so that the regime it promises can be checked without a GPU (head_inputs).  The GPU tests set the
parameters, run the batch and read the head's real inputs (logits, mean, P) back: the float64 / float32 difference of the encoder moves the
inputs by ~1e-5 of their scale, which changes no regime, and the comparison itself never uses the CPU encoder.

Kinds
  mild     the scaling of make() of tests/test_gpu_moe.py: W_moe ~ 0.05 N(0, 1), b_moe ~ 0.1 N(0, 1), b_logits ~ 0.5 N(0, 1); every softmax away
           from saturation; random labels
  trained  what a trained head looks like.  Gate: W_logits scaled and b_logits set so that the logits are centred per expert with a standard
           deviation of 25 over the data set -- each row has one chosen expert (the arg-max), the others are e^-25 .. e^-100 below it.  The last
           max(1, E / 8) experts are DEAD: b_logits = -250 there, a gate weight that is 0.0 in float32 (and 1e-109 in the oracle), and their
           outputs are independent of everybody else's, as an expert's are that no row ever trained.  The live experts agree with each other up to
           15 % (W_moe = c (V[:, o] + 0.15 N(0, 1))): c sets the median top-two gap of the chosen expert's outputs to 30.  Labels: the chosen
           expert's arg-max in ~90 % of the rows; in every tenth row a wrong label, alternately the runner-up (a margin of ~30) and an output that
           a dead expert favours and the live ones do not (a margin of 60 .. 150: its probability underflows -- p < 1e-30 -- while dq = dL/dq of
           that dead expert is ~1e21 s[e, label]: the 0 . 1e21 of the gate's backward).
Classification labels are one-hot, regression labels N(0, 1)."""
import functools

import numpy as np

import dmvae_oracle as O
import moe_oracle as MO

f64 = np.float64
r32 = lambda a: np.asarray(a).astype(np.float32).astype(f64)

SMALL = dict(input_dim=64, enc_layers=(128,), head_dim=128, dec_layers=(128,))
MAX_BATCH, N, N_DATA = 100, 93, 137          # a 128-row plan; 93 real rows: the last workgroup (4 rows) holds one
SHAPES = ((5, 7, 8), (64, 16, 8), (40, 17, 33), (16, 64, 24), (256, 4, 4), (3, 33, 70), (2, 1, 5))      # (E, O, D)
KINDS = ("mild", "trained")
GATE_SCALE, MARGIN_NATS, DEAD_BIAS, LIVE_NOISE = 25.0, 30.0, -250.0, 0.15


def ocfg(shape, layers=SMALL):
    E, Od, D = shape
    return O.Config(layers["input_dim"], D, E, layers["enc_layers"], layers["head_dim"], layers["dec_layers"], "binary")


def n_dead(E):
    return max(1, E // 8)


def case_id(shape, kind, classification, featLearn):
    return "%dx%dx%d-%s-%s-%s" % (shape + (kind, "cls" if classification else "reg", "feat" if featLearn else "x"))


@functools.lru_cache(maxsize=None)
def get_case(shape, kind, classification, featLearn):
    """dict(params: every tensor of the engine, float32-representable float64; X [N_DATA, 64] float32; Y [N_DATA, O] float32; perm int32 [N_DATA])"""
    assert kind in KINDS
    E, Od, D = shape
    cfg = ocfg(shape)
    rng = np.random.RandomState(1000 * KINDS.index(kind) + 100 * classification + 10 * featLearn + E + Od + D)
    I = SMALL["input_dim"]
    X = (rng.rand(N_DATA, I) * (rng.rand(N_DATA, I) < 0.4)).astype(np.float32)
    p = {k: r32(v) for k, v in O.init_params(cfg, 5).items()}
    if featLearn:
        # one collapsed latent dimension, the last: mean = 0.0 exactly in every row -- the edge of the relu gate [mean > 0] of gmu
        p["W_mean"][:, D - 1] = 0.0
        p["b_mean"][D - 1] = 0.0
    a = O.encode(p, cfg, X.astype(f64))
    inp = np.maximum(a["mean"], 0.0) if featLearn else X.astype(f64)
    n_in = inp.shape[1]
    W0 = rng.randn(E, Od, n_in).transpose(2, 0, 1)                     # [in][E][O], drawn as the engine draws regression_weights
    if kind == "mild":
        p["W_moe"] = 0.05 * W0.reshape(n_in, E * Od)
        p["b_moe"] = 0.1 * rng.randn(E * Od)
        p["b_logits"] = 0.5 * rng.randn(E)
        cls = rng.randint(0, Od, N_DATA)
    else:
        dead = np.arange(E) >= E - n_dead(E)
        raw = a["ch"] @ p["W_logits"]
        cen = raw - raw.mean(0)
        gam = GATE_SCALE / cen[:, ~dead].std()
        p["W_logits"] = gam * p["W_logits"]
        p["b_logits"] = -gam * raw.mean(0) + DEAD_BIAS * dead
        chosen = np.argmax(np.where(dead[None], -np.inf, gam * cen), axis=1)
        V = rng.randn(n_in, Od)
        W = np.where(dead[None, :, None], W0, V[:, None, :] + LIVE_NOISE * W0)
        rawP = np.einsum("bi,ieo->beo", inp, W)
        cenP = rawP - rawP.mean(0)
        own = cenP[np.arange(N_DATA), chosen]                         # [N_DATA, O]: each row's chosen expert
        if Od > 1:
            srt = np.sort(own, axis=1)
            c = MARGIN_NATS / np.median(srt[:, -1] - srt[:, -2])
        else:
            c = MARGIN_NATS / own.std()
        noise = 0.1 * rng.randn(E, Od)
        p["W_moe"] = (c * W).reshape(n_in, E * Od)
        p["b_moe"] = (-c * rawP.mean(0) + noise).reshape(E * Od)
        Pfull = c * cenP + noise[None]
        own = Pfull[np.arange(N_DATA), chosen]
        order = np.argsort(own, axis=1)
        cls = order[:, -1].copy()
        wrong = np.flatnonzero(np.arange(N_DATA) % 10 == 3)
        if Od > 1:
            cls[wrong[0::2]] = order[wrong[0::2], -2]                 # the runner-up: a margin of ~30
            for b in wrong[1::2]:                                     # the output a dead expert favours, where the chosen expert's margin against it is largest
                ts = np.argmax(Pfull[b, dead], axis=1)
                t = ts[np.argmax(own[b].max() - own[b, ts])]
                cls[b] = t if t != order[b, -1] else order[b, 0]      # (or, should every dead expert agree with the chosen one, the least-favoured output)
    Y = MO.classification_labels(cls, Od) if classification else rng.randn(N_DATA, Od)
    p = {k: r32(v) for k, v in p.items()}
    perm = rng.permutation(N_DATA).astype(np.int32)
    return dict(shape=shape, kind=kind, classification=classification, featLearn=featLearn, params=p, X=X, Y=Y.astype(np.float32), perm=perm)


def head_inputs(case, n=N):
    """the head's inputs of the case's batch (rows perm[:n]) from the float64 encoder, rounded to float32: logits [n, E], mean [n, D], P [n, E, O], Y"""
    E, Od, D = case["shape"]
    p, idx = case["params"], case["perm"][:n]
    Xb = case["X"][idx].astype(f64)
    a = O.encode(p, ocfg(case["shape"]), Xb)
    inp = np.maximum(r32(a["mean"]), 0.0) if case["featLearn"] else Xb
    P = r32(MO.expert_outputs(p, inp, E, Od))
    return dict(logits=r32(a["logits"]), mean=r32(a["mean"]), P=P, Y=case["Y"][idx].astype(f64))


# ------------------------------------------------------------------------------------------------------------------ oracle and yardstick on given inputs
def oracle(logits, P, Y, classification, inv_B, mean=None, W=None, bias=None):
    """float64: the head on exactly these inputs.  P [n, E, O]; mean / W / bias (featLearn): gmu and P_fl = relu(mean) . W + bias as well (the head
    itself runs on the P it is given)."""
    logits, P, Y = np.asarray(logits, f64), np.asarray(P, f64), np.asarray(Y, f64)
    n, E, Od = P.shape
    q = O.softmax(logits)
    r = MO.head_forward(P, q, Y, classification)
    dP, dq = MO.head_backward(r, classification, inv_B)
    out = dict(q=q, pred=r["pred"], dP=dP, dq=dq, dlogits=MO.dlogits_from(q, dq), loss_rows=r["loss_rows"], err_rows=r["err_rows"],
               loss=float(r["loss_rows"].sum() * inv_B), err=float(r["err_rows"].sum() * (1.0 if classification else inv_B)))
    if mean is not None:
        mean, W, bias = np.asarray(mean, f64), np.asarray(W, f64), np.asarray(bias, f64)
        out["P_fl"] = (np.maximum(mean, 0.0) @ W + bias[None]).reshape(n, E, Od)
        out["gmu"] = (dP.reshape(n, E * Od) @ W.T) * (mean > 0)
    return out


def yardstick(logits, P, Y, classification, inv_B, mean=None, W=None, bias=None):
    return MO.head_f32(P, logits, Y, classification, inv_B, mean, W, bias)


# ------------------------------------------------------------------------------------------------------------------ the tolerance rule
# the project's bars: the prediction as tests/test_gpu_moe.py::test_row_kernel_predict_against_the_oracle holds it, the gradients as
# ::test_fp32_step_against_the_oracle holds them (1e-4 of the tensor's largest entry), the batch scalars as the predict test holds its loss
MARGIN = 2.0
FORWARD, GRADIENTS, SCALARS = ("pred", "P_fl"), ("dP", "dlogits", "gmu"), ("loss", "err")


def yard_error(oracle_v, yard_v):
    return float(np.max(np.abs(np.asarray(yard_v, f64) - np.asarray(oracle_v, f64))))


def project_bar(name, oracle_v):
    """(rtol, atol) without the yardstick's help"""
    m = float(np.max(np.abs(oracle_v)))
    if name in FORWARD:
        return 1e-5, 1e-5 * max(1.0, m)
    if name in GRADIENTS:
        return 0.0, 1e-4 * m
    assert name in SCALARS, name
    return 0.0, 1e-5 * max(1.0, m) * 10


def tolerance(name, oracle_v, yard_v):
    """(rtol, atol): the project's bar, its absolute part raised to MARGIN times the yardstick's own error where that is larger.  The factor 2 is the
    only margin (helpers/trained_latents.py): the kernel's order of additions is not the yardstick's."""
    rtol, atol = project_bar(name, oracle_v)
    return rtol, max(atol, MARGIN * yard_error(oracle_v, yard_v))


def within(name, got, oracle_v, yard_v, tol=None):
    """does `got` meet tolerance(name, ...)?  -> (ok, max |got - oracle|, max |yard - oracle|)"""
    rtol, atol = tolerance(name, oracle_v, yard_v) if tol is None else tol
    got, ref = np.asarray(got, f64), np.asarray(oracle_v, f64)
    fin = bool(np.all(np.isfinite(got)))
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
        ok = fin and bool(np.all(err <= atol + rtol * np.abs(ref)))
    return ok, (float(np.max(err)) if fin else float("inf")), yard_error(oracle_v, yard_v)


def top_two_gap(p):
    if p.shape[1] < 2:
        return np.full(p.shape[0], np.inf)
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


def clear_rows(p_oracle, p_yard):
    """rows whose top-two gap in the oracle's p exceeds four times the yardstick's error in p: the arg-max is the oracle's there"""
    return top_two_gap(p_oracle) > 4.0 * yard_error(p_oracle, p_yard)


def bf16_ulp(x):
    """one unit in the last place of the bf16 numbers of x's binade (8 significant bits)"""
    ax = np.maximum(np.abs(np.asarray(x, f64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)
