"""Float64 restatement of the reference's mixture-of-experts head (code/models.py) on top of dmvae_oracle.

Every formula cites the models.py line it restates.  Shapes: B rows, E experts (= the gate's clusters), O outputs.
W_moe is stored as the library stores it, [in][E*O] with column e*O + o (regression_weights[e][o][i] = W_moe[i][e*O + o]),
b_moe as [E*O] (regression_biases[o][e] = b_moe[e*O + o])."""
import numpy as np

import dmvae_oracle as O


def expert_input(a, X, featLearn):
    # models.py:57-66: inp2cls = relu(vae.mean) with featLearn, else X
    return np.maximum(a["mean"], 0.0) if featLearn else X


def head_forward(P, q, Y, classification):
    """P [B, E, O] expert predictions (models.py:73-78, transposed), q [B, E] gate (vae.cluster_probs, :72).
    Returns a dict with the per-row loss / error and the prediction."""
    r = {"P": P, "q": q, "Y": Y}
    if classification:
        m = P.max(axis=2, keepdims=True)
        s = np.exp(P - m)
        s = s / s.sum(axis=2, keepdims=True)                    # :84-86 softmax over the outputs of each expert
        u = np.sum(s * q[:, :, None], axis=1)                   # :88-90
        p = u / u.sum(axis=1, keepdims=True)                    # :91-93
        r.update(s=s, u=u, p=p)
        r["loss_rows"] = -np.sum(Y * np.log(p + 1e-20), axis=1) * 1000.0      # :141-143 (before the mean)
        top = np.argmax(p, axis=1)                              # :95-99 tf.nn.top_k: first index on ties
        r["pred"] = p
        r["err_rows"] = np.sum(np.abs(Y - np.eye(Y.shape[1])[top]), axis=1) / 2       # :101-103
    else:
        y = np.sum(P * q[:, :, None], axis=1)                   # :106-108
        r["pred"] = y
        d2 = np.sum((y - Y) ** 2, axis=1)
        r["loss_rows"] = 0.5 * d2                               # :145-147: 0.5 * mean_{b,o} * O
        r["err_rows"] = d2                                      # :110-112: mean_{b,o} * O
    return r


def head_backward(r, classification, inv_B):
    """gradients of inv_B * sum_b loss_rows: dP [B, E, O], dq [B, E]"""
    P, q, Y = r["P"], r["q"], r["Y"]
    if classification:
        s, u, p = r["s"], r["u"], r["p"]
        gp = -1000.0 * inv_B * Y / (p + 1e-20)
        U = u.sum(axis=1, keepdims=True)
        gu = (gp - np.sum(gp * p, axis=1, keepdims=True)) / U
        dq = np.sum(s * gu[:, None, :], axis=2)
        ds = q[:, :, None] * gu[:, None, :]
        dP = s * (ds - np.sum(s * ds, axis=2, keepdims=True))
    else:
        res = inv_B * (r["pred"] - Y)
        dP = q[:, :, None] * res[:, None, :]
        dq = np.sum(P * res[:, None, :], axis=2)
    return dP, dq


def expert_outputs(p, inp, E, Od):
    W = p["W_moe"].reshape(-1, E, Od)                           # [in][E][O]
    return np.einsum("bi,ieo->beo", inp, W) + p["b_moe"].reshape(E, Od)[None]


def forward(p, cfg, X, eps, Y, E, Od, featLearn, classification, lossVAE, kl_ratio=1.0, mode="exact", gumbel=None):
    """the whole MoE model's loss (models.py:137-163): loss = loss_moe + lossVAE * vae.loss"""
    a = O.forward(p, cfg, X, eps, kl_ratio=kl_ratio, mode=mode, gumbel=gumbel)
    inp = expert_input(a, X, featLearn)
    P = expert_outputs(p, inp, E, Od)
    r = head_forward(P, a["q"], Y, classification)               # gate = softmax(logits) in both modes (base_models.py:249)
    B = X.shape[0]
    a["moe"] = r
    a["inp"] = inp
    a["loss_moe"] = r["loss_rows"].sum() / B
    a["error"] = r["err_rows"].sum() if classification else r["err_rows"].sum() / B
    a["loss_total"] = a["loss_moe"] + (a["loss"] if lossVAE else 0.0)
    return a


def heads_trunk_backward(p, cfg, a, dmean, dlogits, g):
    """adds the gradients of extra upstream terms dmean / dlogits through the two heads and the trunk (base_models.py:218-249)"""
    g["W_mean"] = g["W_mean"] + a["zh"].T @ dmean
    g["b_mean"] = g["b_mean"] + dmean.sum(0)
    g["W_logits"] = g["W_logits"] + a["ch"].T @ dlogits
    g["b_logits"] = g["b_logits"] + dlogits.sum(0)
    dzh = (dmean @ p["W_mean"].T) * (a["zh"] > 0)
    dch = (dlogits @ p["W_logits"].T) * (a["ch"] > 0)
    ne = len(cfg.enc_layers)
    trunk = a["enc%d" % (ne - 1)]
    g["W_zh"] = g["W_zh"] + trunk.T @ dzh
    g["b_zh"] = g["b_zh"] + dzh.sum(0)
    g["W_ch"] = g["W_ch"] + trunk.T @ dch
    g["b_ch"] = g["b_ch"] + dch.sum(0)
    dh = dzh @ p["W_zh"].T + dch @ p["W_ch"].T
    for i in reversed(range(ne)):
        dy = dh * (a["enc%d" % i] > 0)
        xin = a["enc%d" % (i - 1)] if i > 0 else a["x"]
        g["W_enc%d" % i] = g["W_enc%d" % i] + xin.T @ dy
        g["b_enc%d" % i] = g["b_enc%d" % i] + dy.sum(0)
        if i > 0:
            dh = dy @ p["W_enc%d" % i].T
    return g


def backward(p, cfg, a, E, Od, featLearn, classification, lossVAE):
    """gradient of loss_total w.r.t. every trainable: TF's minimize over the union of the VAE's and the experts' variables"""
    B = a["x"].shape[0]
    gv = O.backward(p, cfg, a)
    g = {k: (v if lossVAE else np.zeros_like(v)) for k, v in gv.items()}
    dP, dq = head_backward(a["moe"], classification, 1.0 / B)
    q = a["q"]
    dlogits = q * (dq - np.sum(q * dq, axis=1, keepdims=True))   # softmax backward, not scaled by kl_ratio
    inp = a["inp"]
    dPf = dP.reshape(B, E * Od)
    g["W_moe"] = inp.T @ dPf
    g["b_moe"] = dPf.sum(0)
    dmean = np.zeros_like(a["mean"])
    if featLearn:
        dmean = (dPf @ p["W_moe"].T) * (a["mean"] > 0)
    return heads_trunk_backward(p, cfg, a, dmean, dlogits, g)


# ---- labels (includes/utils.py:37-74 of the reference)
def classification_labels(classes, n_classes):
    """one-hot over the dataset's classes"""
    return np.eye(n_classes)[np.asarray(classes, dtype=np.int64)]


def dlogits_from(q, dq):
    """softmax backward of the gate, float64: dlogits = q (dq - sum_e q dq)"""
    q, dq = np.asarray(q, np.float64), np.asarray(dq, np.float64)
    return q * (dq - np.sum(q * dq, axis=1, keepdims=True))


# ---- the float32 yardstick: csrc/moe_head.hip restated in NumPy float32, in the kernel's order of operations
def head_f32(P, logits, Y, classification, inv_B, mean=None, W=None, bias=None):
    """moe_head_kernel's own algebra in float32: max-subtracted gate softmax and expert softmaxes, u, U, p, gp, gpp, g, per-expert dq and dP,
    qdq, dlogits; with mean / W / bias (featLearn) P = relu(mean) . W + bias accumulated over d, and gmu.  Every sum (over e, o, d, the batch) is a
    SEQUENTIAL float32 accumulation: the kernel's lane-blocked and shuffled orders should do no worse.  exp and log as the kernel takes them
    (__expf(x) = exp2(fl(x log2 e)), __logf(x) = fl(log2 x) ln 2; helpers/trained_latents.py: _Arith).  Shares nothing with head_forward /
    head_backward but the inputs.  P [B, E, O] (None with featLearn: the head then runs on P_fl, its own product), logits [B, E], Y [B, O], W [D, E*O], bias [E*O], mean [B, D].
    Returns float64 copies of the float32 results: P, P_fl (featLearn), q, pred, dP, dq, dlogits, loss_rows, err_rows, loss, err (the batch scalars of
    moe_finalize_kernel: inv_B sum loss_rows; classification: sum err_rows, regression: inv_B sum err_rows) and, featLearn, gmu."""
    from trained_latents import _Arith
    f32 = np.float32
    A = _Arith(f32)
    lg, Y = np.asarray(logits).astype(f32), np.asarray(Y).astype(f32)
    B, E = lg.shape
    Od = Y.shape[1]
    inv_B = f32(inv_B)
    if mean is not None:
        mean, W, bias = np.asarray(mean).astype(f32), np.asarray(W).astype(f32), np.asarray(bias).astype(f32)
        x = np.maximum(mean, f32(0))
        P_fl = A.seq(mean.shape[1] + 1, lambda d: np.broadcast_to(bias[None], (B, E * Od)).astype(f32) if d == 0 else x[:, d - 1, None] * W[None, d - 1])
        P_fl = P_fl.reshape(B, E, Od)
    P = P_fl if P is None else np.asarray(P).astype(f32).reshape(B, E, Od)
    ge = A.exp(lg - lg.max(1, keepdims=True))
    ginv = f32(1) / A.seq(E, lambda e: ge[:, e])
    q = ge * ginv[:, None]
    out = dict(P=P, q=q)
    if mean is not None:
        out["P_fl"] = P_fl
    if classification:
        ex = A.exp(P - P.max(2, keepdims=True))
        s = ex * (f32(1) / A.seq(Od, lambda o: ex[:, :, o]))[:, :, None]
        u = A.seq(E, lambda e: q[:, e, None] * s[:, e])
        iU = f32(1) / A.seq(Od, lambda o: u[:, o])
        pr = u * iU[:, None]
        lp = A.log(pr + f32(1e-20))
        loss_rows = f32(1000) * A.seq(Od, lambda o: -(Y[:, o] * lp[:, o]))
        top = np.argmax(pr, axis=1)                                      # first index on ties
        hot = (np.arange(Od)[None] == top[:, None]).astype(f32)
        err_rows = f32(0.5) * A.seq(Od, lambda o: np.abs(Y[:, o] - hot[:, o]))
        gp = (f32(-1000) * inv_B) * Y / (pr + f32(1e-20))
        gpp = A.seq(Od, lambda o: gp[:, o] * pr[:, o])
        g = (gp - gpp[:, None]) * iU[:, None]
        sg = A.seq(Od, lambda o: s[:, :, o] * g[:, None, o])            # [B, E]: sum_o s g, which is dq as well
        dq = sg
        dP = (q[:, :, None] * s) * (g[:, None, :] - sg[:, :, None])
        pred = pr
    else:
        u = A.seq(E, lambda e: q[:, e, None] * P[:, e])
        r = u - Y
        l = A.seq(Od, lambda o: r[:, o] * r[:, o])
        loss_rows, err_rows = f32(0.5) * l, l
        g = inv_B * r
        dq = A.seq(Od, lambda o: P[:, :, o] * g[:, None, o])
        dP = q[:, :, None] * g[:, None, :]
        pred = u
    qdq = A.seq(E, lambda e: q[:, e] * dq[:, e])
    dl = q * (dq - qdq[:, None])
    loss = A.seq_rows(loss_rows) * inv_B
    err = A.seq_rows(err_rows) * (f32(1) if classification else inv_B)
    out.update(pred=pred, dP=dP, dq=dq, dlogits=dl, loss_rows=loss_rows, err_rows=err_rows, loss=loss, err=err)
    if mean is not None:
        dPf = dP.reshape(B, E * Od)
        acc = A.seq(E * Od, lambda c: dPf[:, c, None] * W[None, :, c])
        out["gmu"] = np.where(mean > 0, acc, f32(0))
    for k, v in out.items():
        assert np.asarray(v).dtype == f32, (k, np.asarray(v).dtype)
    return {k: (float(v) if np.ndim(v) == 0 else np.asarray(v, np.float64)) for k, v in out.items()}
