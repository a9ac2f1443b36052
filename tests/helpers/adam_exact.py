"""A float32 oracle of the fused weight-gradient + Adam epilogue (DMVAE_EPI_ADAM, dmvae_gemm_grouped_dw_adam) that is EXACT by construction,
the arena layout its tests use and the table of cases tests/test_gpu_dw_adam_forms.py runs (the conditions are checked on the CPU by
tests/test_adam_exact_host.py).  No GPU, no library here.

Why exact: the gradients come from the integer operands of gemm_exact.py -- dW = X^T dY and db = sum_k dY[k][n] are integers below 2^24,
exact in fp32 for any tile, ring depth or summation order -- and the update restates adam_elem<false> (csrc/common.h) one correctly
rounded float32 operation per line, in its order, without fused multiply-add.  The kernel compiles that function under contract(off)
with IEEE sqrtf and division (the library is built without any fast-math flag: deep-mixture-vae_amd/build.py), so with ieee = 1 or
without a bf16 shadow the new param / m / v must have the oracle's BITS, and the shadow the bits of the new param rounded to bf16,
ties to even.  grad_scale is 0.5 or 1: g * grad_scale is exact too."""
import collections
import math

import numpy as np

import gemm_exact as GX

F = np.float32
LR, B1, B2, EPS = F(0.002), F(0.9), F(0.999), F(1e-8)
T_STEP = 3                                              # the update's t (state->adam_t, already advanced): any t >= 3
EINVAL = -1                                             # DMVAE_EINVAL (include/dmvae_hip.h)
EPI_ADAM = 8
GAP = 20                                                # elements between two tensors of an arena: a multiple of 4 (quads), not of 16
LDO_PAD = 32                                            # leading dimension of a weight = N + LDO_PAD (GX.PAD["f32"])
SHADOW_SENT_BITS = GX.SENT_BF16_BITS                    # prefill of the bf16 shadow arena
GRAD_SENT_BITS = GX.NAN_F32_BITS                        # prefill of the gradient arena


def lr_t_double(t, lr=LR, b1=B1, b2=B2):
    """adam_lr_t (csrc/common.h) before its rounding to float32: float32 inputs widened to double"""
    lr, b1, b2 = float(lr), float(b1), float(b2)
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def lr_t(t, lr=LR, b1=B1, b2=B2):
    return F(lr_t_double(t, lr, b1, b2))


def lr_t_margin(t, lr=LR, b1=B1, b2=B2):
    """distance of the double value from the nearest float32 rounding boundary, in float32 ulps (0.5 = as far as it gets): the device
    evaluates the same expression with its own pow / sqrt, a few double ulps (1e-16 relative) from the host's -- the two round to the
    same float32 unless this margin is of that order"""
    x = lr_t_double(t, lr, b1, b2)
    r = F(x)
    ulp = float(np.spacing(r))
    return 0.5 - abs(x - float(r)) / ulp


def adam_f32(p, m, v, g, gscale, lrt, b1=B1, b2=B2, eps=EPS):
    """adam_elem<false>: every line one float32 operation, rounded to nearest even (NumPy float32 arithmetic, sqrt and division are
    IEEE); returns the new (p, m, v)"""
    p, m, v, g = (np.asarray(a, dtype=F) for a in (p, m, v, g))
    gscale, lrt, b1, b2, eps = F(gscale), F(lrt), F(b1), F(b2), F(eps)
    one = F(1.0)
    gj = g * gscale
    c1 = one - b1
    m1 = b1 * m
    m2 = c1 * gj
    mn = m1 + m2
    c2 = one - b2
    v1 = b2 * v
    v2a = c2 * gj
    v2 = v2a * gj
    vn = v1 + v2
    num = lrt * mn
    root = np.sqrt(vn)
    den = root + eps
    quo = num / den
    pn = p - quo
    assert all(a.dtype == F for a in (pn, mn, vn))
    return pn, mn, vn


def bf16_bits(x):
    """float32 -> the uint16 pattern of the nearest bf16, ties to even (GX.bf16_round_bits keeps the same 16 bits in a float)"""
    return (GX.bf16_round_bits(x).astype(F).view(np.uint32) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ problems
Prob = collections.namedtuple("Prob", "M N K bias")     # dW [M][N] = X^T dY over K rows; bias: the fused db [N] (out2) or none


def gradients(q):
    """(problem of gemm_exact with the operands in memory layout, dW [M][N] float32, db [N] float32)"""
    p = GX.make("dw_store_db", q.M, q.N, q.K)
    dW, db = p.expected["out"][0], p.expected["out2"][0].reshape(q.N)
    return p, (dW + 0.0).astype(F), (db + 0.0).astype(F)


# ------------------------------------------------------------------------------------------------ arenas
class Layout:
    """One layout for the five arenas (param, grad, m, v, bf16 shadow): a guard band of GX.GUARD elements, then per problem the weight
    [M][ldo] (ldo = N + pad: pad columns belong to no tensor) and, with a bias, [N]; GAP elements behind each; then the extra segment
    [seg_off, seg_off + seg_n), a gap and the closing guard band.  Offsets count from the arena's first element (the guard's)."""

    def __init__(self, probs, pad=LDO_PAD, seg_n=0):
        self.probs, self.seg_n = tuple(probs), seg_n
        off = GX.GUARD
        self.w_off, self.b_off, self.ldo = [], [], []
        for q in self.probs:
            ldo = q.N + pad
            self.w_off.append(off)
            self.ldo.append(ldo)
            off += q.M * ldo + GAP
            if q.bias:
                self.b_off.append(off)
                off += q.N + GAP
            else:
                self.b_off.append(None)
        self.seg_off = off
        off += seg_n + GAP
        self.n = off + GX.GUARD
        assert all(o % 4 == 0 for o in self.w_off + [b for b in self.b_off if b is not None] + [self.seg_off, self.n]) and all(l % 4 == 0 for l in self.ldo)

    def w_index(self, i):
        q = self.probs[i]
        return self.w_off[i] + np.arange(q.M)[:, None] * self.ldo[i] + np.arange(q.N)[None, :]

    def b_index(self, i):
        return None if self.b_off[i] is None else self.b_off[i] + np.arange(self.probs[i].N)

    def seg_index(self):
        return self.seg_off + np.arange(self.seg_n)

    def tensors(self):
        """index arrays of every tensor the launch updates, in launch order: weights, biases (the segment is apart)"""
        out = []
        for i in range(len(self.probs)):
            out.append(self.w_index(i))
            if self.b_off[i] is not None:
                out.append(self.b_index(i))
        return out


def quads_distinct(a, idx):
    """no two quads of tensor a[idx] alike (idx: rows of a multiple of 4 elements)"""
    q = np.ascontiguousarray(a[idx].reshape(-1, 4))
    return len(np.unique(q.view(np.dtype((np.void, 16))))) == len(q)


def initial_state(lay, seed):
    """param ~ N(0, 1), m ~ N(0, 1e-2), v = |N(0, 1)| 1e-3 in EVERY element of the arenas (pads, gaps and guards too: their bits must
    survive), all nonzero and different; grad: a NaN pattern, with the segment's gradient ~ N(0, 1) stored; shadow: 7.0"""
    rng = np.random.RandomState(seed)
    st = {"param": rng.randn(lay.n).astype(F), "m": (rng.randn(lay.n) * 1e-2).astype(F), "v": (np.abs(rng.randn(lay.n)) * 1e-3).astype(F)}
    assert all((a != 0).all() and np.isfinite(a).all() for a in st.values())
    for idx in lay.tensors() + ([lay.seg_index()] if lay.seg_n else []):
        assert quads_distinct(st["m"], idx) and quads_distinct(st["v"], idx) and quads_distinct(st["param"], idx)
    g = np.full(lay.n, GRAD_SENT_BITS, dtype=np.uint32).view(F).copy()
    if lay.seg_n:
        g[lay.seg_index()] = rng.randn(lay.seg_n).astype(F)
    st["grad"] = g
    st["shadow"] = np.full(lay.n, SHADOW_SENT_BITS, dtype=np.uint16)
    return st


def updated_elements(lay):
    """(flat indices of every element the launch updates -- tensors, then the segment --, their gradient as float32)"""
    idx, g = [], []
    for i, q in enumerate(lay.probs):
        _, dW, db = gradients(q)
        idx.append(lay.w_index(i).reshape(-1))
        g.append(dW.reshape(-1))
        if q.bias:
            idx.append(lay.b_index(i))
            g.append(db)
    return np.concatenate(idx), np.concatenate(g)


def expected_arenas(lay, init, gscale, lrt, shadow, store_grad, update=None):
    """the five arenas after the launch.  update(p, m, v, g) -> (p, m, v): the float32 oracle unless the caller brings another
    yardstick (the stand-alone kernel's results, for the hardware square-root mode).  Whatever is no tensor and not the segment
    keeps its bits; the shadow arena is written only when there is one, the gradient arena only with store_grad, and then only the
    tensors' elements (the segment's gradient is rewritten with its own value)."""
    exp = {k: a.copy() for k, a in init.items()}
    idx, g = updated_elements(lay)
    if lay.seg_n:
        idx = np.concatenate([idx, lay.seg_index()])
        g = np.concatenate([g, init["grad"][lay.seg_index()]])
    assert len(np.unique(idx)) == len(idx)
    up = update or (lambda p, m, v, gg: adam_f32(p, m, v, gg, gscale, lrt))
    pn, mn, vn = up(init["param"][idx], init["m"][idx], init["v"][idx], g)
    exp["param"][idx], exp["m"][idx], exp["v"][idx] = pn, mn, vn
    if shadow:
        exp["shadow"][idx] = bf16_bits(pn)
    if store_grad:
        exp["grad"][idx] = g
    return exp, idx, g


# ------------------------------------------------------------------------------------------------ the case table
MODES = collections.OrderedDict((
    ("ieee", dict(shadow=True, ieee=1)),                # bf16 shadow, IEEE quotient: the oracle's bits
    ("noshadow", dict(shadow=False, ieee=0)),           # param_bf16 = NULL: IEEE whatever ctx.ieee says: the oracle's bits
    ("fast", dict(shadow=True, ieee=0)),                # production: hardware sqrt / rcp: the stand-alone kernel's bits + the float64 bound
))
Case = collections.namedtuple("Case", "id knobs probs mode store_grad gscale pad seg_n rows")
GROUPED_ROW, MULTI_ROW, COLSUM_ROW, ADAM_ROW = "gemm_bf16_grouped_mixed_tiles<L2, E8>", "gemm_bf16_256_dw_multi_kernel<8>", "colsum_slabs", "adam_tf"

P = Prob
# small tiles (knob 6 = 0).  knob 2 = 0: every problem on 64 x 64; knob 2 = 2: the largest tile the shape divides (grouped_launch's
# best_kind): M % 128 == 0 and N % 128 != 0 -> 128 x 64, both % 128 == 0 -> 128 x 128.  K = 64 / 192 / 320: one, three, five K tiles
# (below, at and above the ring depths 2, 3, 4); one problem of each group has no bias gradient; every group is more than one workgroup
G64 = (P(192, 64, 64, True), P(64, 192, 192, True), P(128, 128, 320, False), P(256, 64, 192, True))
G128x64 = (P(128, 64, 64, True), P(256, 192, 192, True), P(128, 192, 320, False), P(256, 64, 320, True))
G128x128 = (P(128, 128, 64, True), P(256, 128, 192, True), P(128, 256, 320, False), P(256, 256, 192, True))
# the macro tile (knob 6 = 2 takes every problem that divides by 256).  K = 128 / 576: the slab column sums of the bias gradient with
# 8 and with 9 rows per slab
M_ONE_A = (P(256, 256, 128, True),)
M_ONE_B = (P(256, 512, 576, True),)
M_MERGED = (P(256, 256, 128, False), P(512, 256, 576, False), P(256, 512, 128, False))         # no bias gradients: one merged grid
M_SEQ = (P(256, 256, 576, False), P(256, 512, 128, True), P(512, 256, 128, False))             # a bias gradient in the middle: three grids in stream order
M_MIXED = (P(256, 256, 128, True), P(256, 512, 576, False), P(512, 256, 576, False), P(192, 64, 192, True))      # the last one stays grouped


def _c(id, knobs, probs, mode, store_grad=0, gscale=0.5, pad=LDO_PAD, seg_n=0, rows=None):
    return Case(id, knobs, probs, mode, store_grad, gscale, pad, seg_n, rows)


def form_cases():
    out = []
    sg = {"ieee": 1, "noshadow": 0, "fast": 1}          # store_grad goes with two of the three modes
    for mode in MODES:
        out.append(_c("t64x64-%s" % mode, {6: 0, 2: 0}, G64, mode, sg[mode], rows={GROUPED_ROW: 1}))
        for nw8 in (0, 1):                              # knob 1 (eight waves for the dense launches' 128-row tiles): the grouped kernel has one form, four waves
            out.append(_c("t128x64-k1=%d-%s" % (nw8, mode), {6: 0, 2: 2, 1: nw8}, G128x64, mode, sg[mode], rows={GROUPED_ROW: 1}))
            out.append(_c("t128x128-k1=%d-%s" % (nw8, mode), {6: 0, 2: 2, 1: nw8}, G128x128, mode, sg[mode], rows={GROUPED_ROW: 1}))
        out.append(_c("planned-%s" % mode, {6: 0, 2: 1}, G128x128, mode, 1 - sg[mode], rows={GROUPED_ROW: 1}))      # the tile planner's own choice
        out.append(_c("m256-one-k128-%s" % mode, {6: 2, 2: 0}, M_ONE_A, mode, sg[mode], rows={COLSUM_ROW: 1, MULTI_ROW: 1}))
        out.append(_c("m256-one-k576-%s" % mode, {6: 2, 2: 0}, M_ONE_B, mode, 1 - sg[mode], rows={COLSUM_ROW: 1, MULTI_ROW: 1}))
        out.append(_c("m256-merged-%s" % mode, {6: 2, 2: 0}, M_MERGED, mode, sg[mode], rows={MULTI_ROW: 1}))
        out.append(_c("m256-seq-%s" % mode, {6: 2, 2: 0}, M_SEQ, mode, sg[mode], rows={COLSUM_ROW: 1, MULTI_ROW: 3}))
        out.append(_c("m256-mixed-%s" % mode, {6: 2, 2: 0}, M_MIXED, mode, sg[mode], rows={COLSUM_ROW: 1, MULTI_ROW: 2, GROUPED_ROW: 1}))
    # context settings that the table above leaves at one value
    out.append(_c("t64x64-ldo=N-ieee", {6: 0, 2: 0}, G64, "ieee", 1, pad=0, rows={GROUPED_ROW: 1}))
    out.append(_c("t128x128-ldo=N-noshadow", {6: 0, 2: 2}, G128x128, "noshadow", 1, pad=0, rows={GROUPED_ROW: 1}))
    out.append(_c("m256-ldo=N-ieee", {6: 2, 2: 0}, M_ONE_A, "ieee", 0, pad=0, rows={COLSUM_ROW: 1, MULTI_ROW: 1}))
    out.append(_c("t128x64-gscale=1-ieee", {6: 0, 2: 2}, G128x64, "ieee", 0, gscale=1.0, rows={GROUPED_ROW: 1}))
    out.append(_c("m256-gscale=1-fast", {6: 2, 2: 0}, M_MIXED, "fast", 0, gscale=1.0, rows={COLSUM_ROW: 1, MULTI_ROW: 2, GROUPED_ROW: 1}))
    return out


SEG_NS = (4, 1024, 4100)                                # one quad | one pass of a 256-thread lead block | more than four blocks' first pass


def segment_cases():
    """the extra arena segment riding a grouped launch (its lead workgroups hold the first ids; the tiles behind them are shifted),
    and with every problem peeled to the macro tile, where it falls to the stand-alone kernel"""
    out = []
    modes = list(MODES)
    for i, n in enumerate(SEG_NS):
        out.append(_c("seg%d-rides-%s" % (n, modes[i]), {6: 0, 2: 2}, G128x64 if i % 2 else G64 + G128x128[:1], modes[i], i % 2, seg_n=n, rows={GROUPED_ROW: 1}))
        out.append(_c("seg%d-peeled-%s" % (n, modes[(i + 1) % 3]), {6: 2, 2: 0}, M_MERGED[:2], modes[(i + 1) % 3], (i + 1) % 2, seg_n=n,
                      rows={MULTI_ROW: 1, ADAM_ROW: 1}))
    out.append(_c("seg4100-rides-mixed-fast", {6: 2, 2: 0}, M_MIXED, "fast", 1, seg_n=4100, rows={COLSUM_ROW: 1, MULTI_ROW: 2, GROUPED_ROW: 1}))
    return out


def all_cases():
    return form_cases() + segment_cases()


def all_probs():
    return sorted({q for c in all_cases() for q in c.probs})


def tile_kind(q, knob2):
    """grouped_launch's best_kind (csrc/gemm_bf16.hip) under knob 2 = 0 / 2: the tile a problem runs on"""
    if knob2 == 0:
        return (64, 64)
    return (128, 128) if (q.M % 128 == 0 and q.N % 128 == 0) else ((128, 64) if q.M % 128 == 0 else (64, 64))
