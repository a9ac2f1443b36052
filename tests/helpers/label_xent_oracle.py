"""The semi-supervised label term of csrc/label_xent.hip, restated: cross-entropy on q(c|x) = softmax(logits) for the rows that carry a label.

  term(logits, y, coef)       float64: l_r = logsumexp(logits_r) - logits_r[y_r] and d_r[k] = coef (q_r[k] - [k == y_r]) for y_r >= 0; rows with
                              y_r == -1 (or a label outside [0, K): the kernel skips them and flags them) contribute nothing
  term_f32(logits, y, coef)   the float32 yardstick: the same formulas in float32 arithmetic, in numpy's order of additions -- what a
                              float32 implementation may lose; the kernel's order is another one (the tolerance rule doubles its error)
  batch_labels(labels, perm, first, n)      y_r = labels[perm[first + r]]

Both return dict(loss_rows [n], d [n][K], labelled [n] bool, correct [n] bool, loss, n_labelled, n_correct, bad [n] bool)."""
import numpy as np

f64 = np.float64
f32 = np.float32


def batch_labels(labels, perm, first, n):
    idx = np.arange(first, first + n) if perm is None else np.asarray(perm)[first:first + n]
    return np.asarray(labels)[idx].astype(np.int64)


def _term(logits, y, coef, ft):
    lg = np.asarray(logits, dtype=ft)
    y = np.asarray(y, dtype=np.int64)
    n, K = lg.shape
    bad = (y < -1) | (y >= K)
    lab = (y >= 0) & ~bad
    loss_rows = np.zeros(n, dtype=ft)
    d = np.zeros((n, K), dtype=ft)
    correct = np.zeros(n, dtype=bool)
    coef = ft(coef)
    for r in np.nonzero(lab)[0]:
        row = lg[r]
        mx = row.max()
        ex = np.exp(row - mx)              # (float32 in: float32 out)
        se = ex.sum(dtype=ft)
        loss_rows[r] = np.log(se) + (mx - row[y[r]])
        q = ex * (ft(1.0) / se) if ft is f32 else ex / se
        onehot = np.zeros(K, dtype=ft)
        onehot[y[r]] = 1
        d[r] = coef * (q - onehot)
        correct[r] = int(np.argmax(row)) == y[r]       # np.argmax: the first index of the largest
    return dict(loss_rows=loss_rows, d=d, labelled=lab, correct=correct, bad=bad, loss=float(loss_rows.astype(f64).sum()),
                n_labelled=int(lab.sum()), n_correct=int(correct.sum()))


def term(logits, y, coef):
    return _term(logits, y, coef, f64)


def term_f32(logits, y, coef):
    return _term(logits, y, coef, f32)


def coefficient(w, inv_B):
    """w * inv_B as the kernel forms it: one float32 product"""
    return float(f32(w) * f32(inv_B))


def mean_xent(logits, y):
    """mean l_r over the labelled rows (float64)"""
    t = term(logits, y, 0.0)
    return t["loss"] / max(1, t["n_labelled"])
