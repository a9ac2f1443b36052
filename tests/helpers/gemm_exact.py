"""Inputs for which the reference of a dense GEMM with a fused epilogue is EXACT, and the table of cases the GPU tests run on them
(tests/test_gpu_gemm_forms.py; the conditions below are checked on the CPU by tests/test_gemm_exact_host.py).  No GPU, no library here.

Why exact: operands are integers in [-2, 2] (exact in bf16), so every fp32 partial sum of a product is an integer below 2^24 -- the
accumulation is exact in any order, for any tile shape, ring depth or K split.  Bias and the LATENT arrays are integers in [-4, 4]:
acc + bias and acc * clv + glv are exact with or without FMA contraction.  A bf16 output is the exact value rounded once, to nearest
even (what the kernels' pack2bf does).  The reconstruction epilogue of the real kind gets operands that make every loss term a multiple
of 2^-5 (see operands_onehot), so the loss partial of a tile is exact in any summation order as well.  The binary kind and the sigmoid
use the hardware exponential: there only the logits are exact."""
import collections
import functools

import numpy as np
import torch

FWD, DX, DW = 0, 1, 2                                   # DMVAE_GEMM_* (include/dmvae_hip.h)
(EPI_BIAS_RELU, EPI_BIAS_F32, EPI_BIAS_RECON, EPI_RELU_MASK, EPI_LATENT, EPI_STORE_F32, EPI_ATOMIC_F32, EPI_BIAS_SIGMOID) = range(8)

K_SET = (64, 128, 192, 320, 576)                        # 1, 2, 3, 5 and 9 K tiles: below, at and above every ring depth (2, 3, 4), with tails
GUARD = 4096                                            # sentinel elements in front of and behind every buffer
PAD = {"bf16": 64, "f32": 32}                           # leading dimension = width + PAD
SENT_BF16_BITS = 0x40E0                                 # 7.0: prefill of bf16 outputs, their pad columns and guards
NAN_BF16_BITS = 0x7FC0                                  # pad columns and guards of bf16 inputs
NAN_F32_BITS = 0x7FC12345                               # a quiet NaN with a payload: f32 inputs' pads, f32 outputs' prefill, pads and guards
RECON_SCALE = 2.0 ** -8                                 # deliberately not 1 / m_valid
LATENT_D = 64

Form = collections.namedtuple("Form", "name bm bn nstage nw knobs short")
# dmvae_debug_set_tile(bm, bn) + knobs; nstage / nw: the instantiation launch_tiled has for it (csrc/gemm_bf16.hip)
FORMS = collections.OrderedDict((f.name, f) for f in (
    Form("64x64", 64, 64, 4, 4, {}, False),
    Form("64x64s2", 64, 64, 2, 4, {7: 1}, True),       # the 2-slot "short-K" ring: K <= 128, FWD / DX, no RECON
    Form("64x128", 64, 128, 3, 4, {}, False),
    Form("128x64w4", 128, 64, 3, 4, {1: 0}, False),
    Form("128x64w8", 128, 64, 3, 8, {1: 1}, False),
    Form("128x128w4", 128, 128, 2, 4, {1: 0}, False),
    Form("128x128w8", 128, 128, 2, 8, {1: 1}, False),
))
KNOB_DEFAULTS = {0: 0, 1: 1, 2: 1, 6: 1, 7: 0, 9: 0, 13: 1, 18: 2}

Pair = collections.namedtuple("Pair", "name layout epi recon_kind split onehot")
PAIRS = collections.OrderedDict((p.name, p) for p in (
    Pair("fwd_bias_relu", FWD, EPI_BIAS_RELU, 0, 1, False),
    Pair("fwd_bias_f32", FWD, EPI_BIAS_F32, 0, 1, False),
    Pair("fwd_recon_real", FWD, EPI_BIAS_RECON, 1, 1, True),
    Pair("fwd_recon_binary", FWD, EPI_BIAS_RECON, 0, 1, True),
    Pair("fwd_sigmoid", FWD, EPI_BIAS_SIGMOID, 0, 1, True),
    Pair("fwd_store", FWD, EPI_STORE_F32, 0, 1, False),
    Pair("dx_store", DX, EPI_STORE_F32, 0, 1, False),
    Pair("dx_relu_mask", DX, EPI_RELU_MASK, 0, 1, False),
    Pair("dx_latent", DX, EPI_LATENT, 0, 1, False),
    Pair("dw_store_db", DW, EPI_STORE_F32, 0, 1, False),       # with the fused bias gradient in out2
    Pair("dw_atomic_s2", DW, EPI_ATOMIC_F32, 0, 2, False),     # split-K onto pre-zeroed out / out2
    Pair("dw_atomic_s4", DW, EPI_ATOMIC_F32, 0, 4, False),
))
INEXACT = ("fwd_recon_binary", "fwd_sigmoid")           # hardware exp / rcp: exact logits, the rest against float64 and the 64x64 form

Case = collections.namedtuple("Case", "id form pair M N Ks")


def _ks(pair, ks):
    """K of a launch: every K slice of a split launch is as deep as an unsplit launch of the set (the ring sees k_split, not K)"""
    return tuple(k * pair.split for k in ks)


def dense_cases():
    """(form, pair) on M = 5 BM, N = 3 BN -- the smallest grid with odd, unequal tile counts, interior and edge tiles -- K looped inside"""
    out = []
    for f in FORMS.values():
        for p in PAIRS.values():
            if f.short and (p.layout == DW or p.epi == EPI_BIAS_RECON):
                continue
            if p.epi == EPI_LATENT and f.bn != LATENT_D:
                continue
            N = LATENT_D if p.epi == EPI_LATENT else 3 * f.bn
            ks = tuple(k for k in K_SET if k <= 128) if f.short else K_SET
            out.append(Case("%s-%s" % (f.name, p.name), f, p, 5 * f.bm, N, _ks(p, ks)))
    return out


SuperCase = collections.namedtuple("SuperCase", "id form pair group_m M N Ks")


def supertile_cases():
    """knob 0 on a 5 x 3 tile grid, whose row count none of 2, 3, 4 divides"""
    out = []
    for fn in ("64x64", "128x64w4", "128x64w8"):
        f = FORMS[fn]
        for pn in ("fwd_bias_relu", "dx_relu_mask"):
            for gm in (2, 3, 4):
                out.append(SuperCase("%s-%s-gm%d" % (fn, pn, gm), f, PAIRS[pn], gm, 5 * f.bm, 3 * f.bn, (64, 320)))
    return out


ThinCase = collections.namedtuple("ThinCase", "id knob rows nw M N Ks")
# the dZ GEMM (LATENT, N = 64, K >= 1024) on 16- / 32-row tiles.  dmvae_gemm takes M in multiples of 64 only, so the smallest odd grid
# of the general tile, M = 320, serves both: twenty 16-row tiles, ten 32-row tiles, five 64-row tiles for the knob 18 = 0 comparison
THIN_CASES = (ThinCase("thin16", 2, 16, 2, 320, LATENT_D, (1024, 1088)), ThinCase("thin32", 1, 32, 4, 320, LATENT_D, (1024, 1088)))

GROUP_FWD = ((128, 128, 192), (128, 64, 64), (64, 192, 320), (192, 128, 576))      # (M, N, K) of the four problems of one grouped call
GROUP_DX = GROUP_FWD
GROUP_DX_STREAM = ((192, 256, 128), (128, 128, 128))    # K = 128, N % 128 == 0, two problems: what the streaming kernel takes (knob 13)
GroupCase = collections.namedtuple("GroupCase", "id pair shapes knobs")


def grouped_cases():
    out = []
    for k2 in (0, 1, 2):
        out.append(GroupCase("fwd_bias_f32-k2=%d" % k2, PAIRS["fwd_bias_f32"], GROUP_FWD, {2: k2}))
        out.append(GroupCase("dx_relu_mask-k2=%d" % k2, PAIRS["dx_relu_mask"], GROUP_DX, {2: k2}))
        out.append(GroupCase("dx_relu_mask-k2=%d-w8" % k2, PAIRS["dx_relu_mask"], GROUP_DX, {2: k2, 9: 8}))
    return out


F32_SHAPE = (320, 192)
F32_KS = (64, 320)


def f32_cases():
    return [Case("f32-%s" % p.name, None, p, F32_SHAPE[0], LATENT_D if p.epi == EPI_LATENT else F32_SHAPE[1], _ks(p, F32_KS)) for p in PAIRS.values()]


# ------------------------------------------------------------------------------------------------ the 256 x 256 macro tile
# (csrc/gemm_bf16_256.hip; tests/test_gpu_gemm256_forms.py.  Knob 6 = 2 sends every shape that divides by 256 to it.)
MACRO = 256
MACRO_SHAPE = (5 * MACRO, 3 * MACRO)                    # the odd, unequal grid of the small forms: interior and edge tiles, a supertile remainder
MACRO_PAIRS = ("fwd_bias_relu", "fwd_store", "dx_store", "dx_relu_mask", "fwd_recon_real", "dw_store_db", "fwd_recon_binary")
MACRO_NOT_INSTANTIATED = ("fwd_bias_f32", "fwd_sigmoid", "dx_latent", "dw_atomic_s2")      # these must stay on the small tiles, exact as before
MacroCase = collections.namedtuple("MacroCase", "id pair M N Ks rows")


def macro_rows(pair):
    """the profiler rows of one dmvae_gemm launch of `pair` on the macro tile (the fused bias gradient of a dW problem: slab column sums first)"""
    rows = ["gemm_bf16_256_kernel<%d, %d>" % (pair.layout, pair.epi)]
    return ["colsum_slabs"] + rows if pair.layout == DW else rows


def macro_cases():
    """every pair the macro tile is instantiated for, on 5 x 3 tiles over the K set and on a single tile with a single K tile"""
    out = []
    for pn in MACRO_PAIRS:
        p = PAIRS[pn]
        out.append(MacroCase("m256-%s" % pn, p, MACRO_SHAPE[0], MACRO_SHAPE[1], K_SET, macro_rows(p)))
        out.append(MacroCase("m256-one-tile-%s" % pn, p, MACRO, MACRO, (64,), macro_rows(p)))
    return out


def macro_fallback_cases():
    """the pairs the macro tile has no instantiation for, at a shape it would take (LATENT with a latent width of 256: out is [M][2 N])"""
    out = []
    for pn in MACRO_NOT_INSTANTIATED:
        p = PAIRS[pn]
        out.append(MacroCase("m256-not-%s" % pn, p, 2 * MACRO, MACRO, _ks(p, (64, 320)), None))
    return out


# column sums of the bf16-rounded output per 256-row tile (GemmArgs::csum_out), (pair, M, N, K): one, three and nine K tiles
CSUM_OUT_CASES = tuple((pn, MACRO_SHAPE[0], MACRO_SHAPE[1], K) for pn in ("dx_relu_mask", "fwd_recon_real", "fwd_recon_binary") for K in (64, 192, 576))
# partials handed to a weight-gradient problem (GemmArgs::csum_in): (M, N, K, csum_rows)
CSUM_IN_CASES = ((256, 768, 128, 1), (512, 256, 192, 2), (256, 512, 320, 5))
CSUM_IN_MERGED = (1, 2)                                 # two of them in ONE call: their bias-gradient workgroups run behind all tiles of the merged grid
CSUM_IN_RANGE = 1000                                    # partials: integers in [-1000, 1000], nothing to do with the column sums of B
# the chain: dY = a dx_relu_mask launch's out [M][N] and its csum_out -> B operand and csum_in of dW [CHAIN_X][N] = X^T dY over K = M rows
CHAIN_DX = ("dx_relu_mask", MACRO_SHAPE[0], MACRO_SHAPE[1], 192)
CHAIN_X = 256
CHAIN_DW = (CHAIN_X, CHAIN_DX[2], CHAIN_DX[1])          # (M, N, K) of that weight-gradient problem: its operands are not a make() problem (chain_problem)
# K slices of a weight-gradient problem into slabs: (M, N, k_split, slices).  Calls: each alone, and the three merged into one grid
SLICE_CASES = ((512, 256, 64, 2), (256, 512, 128, 3), (256, 256, 192, 2), (256, 256, 64, 3), (256, 256, 192, 1))
SLICE_MERGED = (0, 1, 4)                                # two sliced problems of different slice counts and one unsliced problem


def csum_in_partials(M, N, K, rows):
    rng = np.random.RandomState(M + 3 * N + 7 * K + rows)
    return rng.randint(-CSUM_IN_RANGE, CSUM_IN_RANGE + 1, size=(rows, N)).astype(np.float64)


def tile_colsums(out, valid_rows=None, valid_cols=None):
    """float64 column sums per 256-row tile of out [M][N] -> [M / 256][N]; rows / columns at or beyond the valid counts contribute zero"""
    o = np.array(out, dtype=np.float64)
    if valid_rows is not None:
        o[valid_rows:] = 0.0
    if valid_cols is not None:
        o[:, valid_cols:] = 0.0
    return o.reshape(o.shape[0] // MACRO, MACRO, o.shape[1]).sum(1)


def csum_out_expected(p):
    """the exact column sums a macro-tile launch of p leaves: of the expected output rounded to bf16"""
    o = bf16_round(p.expected["out"][0])
    if p.pair.epi == EPI_BIAS_RECON:
        return tile_colsums(o, p.m_valid, p.n_valid)
    return tile_colsums(o)


def colsum_exact_report(addends, tile=MACRO):
    """the condition that makes an f32 column sum exact in ANY order: all addends of a tile's column are multiples of a common quantum q
    (a power of two) and their absolute sum stays below 2^24 q -- every partial sum is then a multiple of q below 2^24 q: representable"""
    a = np.abs(np.asarray(addends, dtype=np.float64))
    nz = a[a != 0]
    ok = {}
    if nz.size == 0:
        return {"(all zero)": True}
    q = 2.0 ** np.floor(np.log2(nz.min()))
    while not (a / q == np.rint(a / q)).all() and q > 2.0 ** -40:
        q /= 2.0
    ok["addends are multiples of a common quantum"] = bool((a / q == np.rint(a / q)).all())
    rows = a.shape[0]
    t = min(tile, rows)
    sums = a[:rows // t * t].reshape(rows // t, t, -1).sum(1)
    ok["sum of |addends| < 2^24 quanta per tile and column"] = bool(sums.max() < 2 ** 24 * q)
    return ok


def chain_problem():
    """(the dx_relu_mask problem, X [K][CHAIN_X] as float64, dW, db): dY = the bf16-rounded expected output of the dx launch"""
    p = make(*CHAIN_DX)
    dY = bf16_round(p.expected["out"][0])
    rng = np.random.RandomState(4242)
    X = rng.randint(-2, 3, size=(p.M, CHAIN_X)).astype(np.float64)
    return p, X, dY, X.T @ dY, dY.sum(0)


def slice_partials(p, k_split, nsl):
    """the exact partial product of every K slice of the dW problem p: [nsl][M][N]"""
    return np.stack([p.A[:, y * k_split:(y + 1) * k_split] @ p.B[y * k_split:(y + 1) * k_split] for y in range(nsl)])


def all_problem_keys():
    """every (pair name, M, N, K) the GPU files generate: what the host test checks"""
    keys = []
    for c in macro_cases() + macro_fallback_cases():
        keys += [(c.pair.name, c.M, c.N, K) for K in c.Ks]
    keys += list(CSUM_OUT_CASES) + [CHAIN_DX]
    keys += [("dw_store_db", M, N, K) for (M, N, K, _) in CSUM_IN_CASES]
    keys += [("dw_store_db", M, N, ks * nsl) for (M, N, ks, nsl) in SLICE_CASES]
    for c in dense_cases() + f32_cases():
        keys += [(c.pair.name, c.M, c.N, K) for K in c.Ks]
    for c in supertile_cases():
        keys += [(c.pair.name, c.M, c.N, K) for K in c.Ks]
    for c in THIN_CASES:
        keys += [("dx_latent", c.M, c.N, K) for K in c.Ks]
    for c in grouped_cases():
        keys += [(c.pair.name, M, N, K) for (M, N, K) in c.shapes]
    keys += [("dx_relu_mask", M, N, K) for (M, N, K) in GROUP_DX_STREAM]
    return sorted(set(keys))


def all_case_ids():
    return ([c.id for c in dense_cases()] + [c.id for c in supertile_cases()] + [c.id for c in THIN_CASES] + [c.id for c in grouped_cases()] +
            [c.id for c in f32_cases()] + [c.id for c in macro_cases()] + [c.id for c in macro_fallback_cases()])


# ------------------------------------------------------------------------------------------------ rounding
def bf16_round(x):
    """float64 -> the bf16 value nearest to it (ties to even), as float64"""
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float32).bfloat16().double().numpy()


def bf16_round_bits(x):
    """the same from the bit pattern, for the host test: add half an ulp (+ the kept lsb, for ties to even), truncate"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ operands
def _distinct_rows(a):
    return len(np.unique(a, axis=0)) == len(a)


def operands_int(M, N, K, rng):
    """logical A [M][K], B [K][N]: integers in [-2, 2]; no two rows of A and no two columns of B alike, so that a swapped fragment,
    a tile read from another tile's place or a transposed pair cannot cancel"""
    A = rng.randint(-2, 3, size=(M, K)).astype(np.float64)
    B = rng.randint(-2, 3, size=(K, N)).astype(np.float64)
    assert _distinct_rows(A) and _distinct_rows(B.T)
    return A, B


def onehot_col(m, K):
    return (37 * m) % K                                 # 37 is prime to every K of the table (64 x 1, 2, 3, 5, 9, 17): a window of K rows visits every column once


def operands_onehot(M, N, K, rng):
    """A has exactly one +-1 per row, at column 37 m mod K (it walks the whole K range, every K tile of the ring contributes), the
    sign flipping every K rows: A . B is then one signed row of B, in [-2, 2].  (At most 2 K such rows exist, so rows repeat at a
    distance of 2 K -- inside an aligned window of 2 K rows, which holds a whole 128-row tile at every K, all rows differ.)"""
    A = np.zeros((M, K))
    m = np.arange(M)
    A[m, onehot_col(m, K)] = np.where((m // K) % 2 == 0, 1.0, -1.0)
    B = rng.randint(-2, 3, size=(K, N)).astype(np.float64)
    assert _distinct_rows(B.T)
    return A, B


GATE_VALUES = np.array([0.0, -0.0, -1.5, -2.0 ** -7, -2.0 ** -126, 2.0 ** -126, 0.5, 1.0, 3.0])      # 2^-126: the smallest normal bf16 (and f32)


class Problem:
    """one GEMM + epilogue: logical operands, their memory layout, the epilogue's inputs and the exact expected outputs (float64)"""


@functools.lru_cache(maxsize=8)
def make(pair_name, M, N, K):
    p = Problem()
    pair = PAIRS[pair_name]
    p.pair, p.M, p.N, p.K = pair, M, N, K
    rng = np.random.RandomState((list(PAIRS).index(pair_name) * 7919 + M * 31 + N * 17 + K) % (2 ** 31))
    p.A, p.B = (operands_onehot if pair.onehot else operands_int)(M, N, K, rng)
    p.A_mem = p.A.T.copy() if pair.layout == DW else p.A          # DW: A = X [K][M]
    p.B_mem = p.B.T.copy() if pair.layout == DX else p.B          # DX: B = W [N][K]
    p.bias = None
    p.aux = {}                                                     # name -> (array, "act" | "f32")
    e = pair.epi
    if e in (EPI_BIAS_RELU, EPI_BIAS_F32):
        p.bias = rng.randint(-4, 5, size=N).astype(np.float64)
    elif e in (EPI_BIAS_RECON, EPI_BIAS_SIGMOID):
        p.bias = rng.randint(-2, 3, size=N).astype(np.float64)    # logits in [-4, 4]
    if e == EPI_BIAS_RECON:
        p.aux["aux0"] = (rng.randint(0, 5, size=(M, N)) / 4.0, "f32")      # targets: multiples of 1/4 in [0, 1]
        p.m_valid, p.n_valid = M - 37, N - 22                      # both cut through a tile, neither a multiple of 4
    if e == EPI_RELU_MASK:
        p.aux["aux0"] = (GATE_VALUES[rng.randint(0, len(GATE_VALUES), size=(M, N))], "act")
    if e == EPI_LATENT:
        for k in ("aux0", "aux1", "aux2"):                         # gmu, glv, clv
            p.aux[k] = (rng.randint(-4, 5, size=(M, N)).astype(np.float64), "f32")
    p.expected = reference(p, np.float64)
    return p


def reference(p, dt):
    """the expected outputs, evaluated in `dt` (float64; float32 gives the same bits -- every intermediate is representable -- which the
    host test checks).  name -> (array as float64, "act" | "f32"); act outputs are rounded to bf16 by the caller when the launch is bf16."""
    pair, M, N = p.pair, p.M, p.N
    A, B = p.A.astype(dt), p.B.astype(dt)
    acc = A @ B
    bias = None if p.bias is None else p.bias.astype(dt)
    aux = {k: v[0].astype(dt) for k, v in p.aux.items()}
    e = pair.epi
    r = {}
    if e == EPI_BIAS_RELU:
        r["out"] = (np.maximum(acc + bias, dt(0)), "act")
    elif e == EPI_BIAS_F32:
        r["out"] = (acc + bias, "f32")
    elif e in (EPI_STORE_F32, EPI_ATOMIC_F32):
        r["out"] = (acc, "f32")
        if pair.layout == DW:
            r["out2"] = (B.sum(0).reshape(1, N), "f32")
    elif e == EPI_RELU_MASK:
        r["out"] = (np.where(aux["aux0"] > 0, acc, dt(0)), "act")
    elif e == EPI_LATENT:
        r["out"] = (np.concatenate([acc + aux["aux0"], acc * aux["aux2"] + aux["aux1"]], axis=1), "act")
    elif e == EPI_BIAS_SIGMOID:
        r["logits"] = (acc + bias, "f32")                          # (not an output of the launch: what its sigmoid is taken of)
    elif e == EPI_BIAS_RECON:
        l = acc + bias
        r["out2"] = (l, "f32")                                     # the logits copy: every row and column, valid or not
        mask = np.zeros((M, N), dtype=bool)
        mask[:p.m_valid, :p.n_valid] = True
        if pair.recon_kind == 1:
            res = l - aux["aux0"]
            r["out"] = (np.where(mask, res * dt(RECON_SCALE), dt(0)), "act")
            r["terms"] = (np.where(mask, dt(0.5) * res * res, dt(0)), "f32")
    return {k: (np.asarray(v[0], dtype=np.float64), v[1]) for k, v in r.items()}


def binary_reference(p, logits):
    """float64 cross entropy terms and gradient of the binary kind from the (exact) logits"""
    x = p.aux["aux0"][0]
    mask = np.zeros((p.M, p.N))
    mask[:p.m_valid, :p.n_valid] = 1.0
    per = np.maximum(logits, 0) - logits * x + np.log1p(np.exp(-np.abs(logits)))
    return per * mask, (1.0 / (1.0 + np.exp(-logits)) - x) * RECON_SCALE * mask


def tile_sums(terms, bm, bn):
    M, N = terms.shape
    return terms.reshape(M // bm, bm, N // bn, bn).sum(axis=(1, 3))


def exactness_report(p):
    """the conditions the exact comparisons rest on, as a dict of booleans (all must hold)"""
    pair, K = p.pair, p.K
    ok = {}
    inb = lambda a, lo, hi: bool((a >= lo).all() and (a <= hi).all() and (a == np.rint(a)).all())
    ok["operands are integers in [-2, 2]"] = inb(p.A, -2, 2) and inb(p.B, -2, 2)
    ok["operands are exact in bf16"] = bool((bf16_round(p.A) == p.A).all() and (bf16_round(p.B) == p.B).all())
    absacc = np.abs(p.A) @ np.abs(p.B)                             # bounds every partial sum of every element, in any order
    ok["|acc| < 2^24 in any order"] = bool(absacc.max() < 2 ** 24) and 4 * K < 2 ** 24
    if p.bias is not None:
        ok["bias: integers in [-4, 4]"] = inb(p.bias, -4, 4)
        ok["|acc| + |bias| < 2^24"] = bool((absacc + np.abs(p.bias)).max() < 2 ** 24)
    if pair.onehot:
        nz = (p.A != 0)
        ok["A: one +-1 per row"] = bool((nz.sum(1) == 1).all() and (np.abs(p.A).sum(1) == 1).all())
        col = np.argmax(nz, axis=1)
        ok["A: the column walks the whole K range"] = (len(set(col[:K])) == min(p.M, K)) and set(col // 64) == set(range(K // 64))
        w = min(2 * K, p.M)
        ok["A: rows differ inside every aligned window of 2 K rows"] = all(_distinct_rows(p.A[s:s + w]) for s in range(0, p.M, w))
        ok["logits in [-4, 4]"] = inb(p.A @ p.B + p.bias, -4, 4)
    else:
        ok["rows of A and columns of B are distinct"] = _distinct_rows(p.A) and _distinct_rows(p.B.T)
    if pair.epi == EPI_RELU_MASK:
        g = p.aux["aux0"][0]
        ok["gates are exact in bf16 and of every kind"] = bool((bf16_round(g) == g).all()) and all(
            bool(((g == v) & (np.signbit(g) == np.signbit(v))).any()) for v in GATE_VALUES)
    if pair.epi == EPI_LATENT:
        ok["latent arrays: integers in [-4, 4]"] = all(inb(p.aux[k][0], -4, 4) for k in ("aux0", "aux1", "aux2"))
        ok["|acc * clv| + |glv| < 2^24"] = bool((absacc * np.abs(p.aux["aux2"][0]) + np.abs(p.aux["aux1"][0])).max() < 2 ** 24)
    if pair.epi == EPI_BIAS_RECON:
        x = p.aux["aux0"][0]
        ok["targets: multiples of 1/4 in [0, 1]"] = inb(4 * x, 0, 4)
        ok["m_valid, n_valid cut a tile, no multiple of 4"] = p.m_valid % 4 != 0 and p.n_valid % 4 != 0 and p.m_valid % 64 != 0 and p.n_valid % 64 != 0
        if pair.recon_kind == 1:
            t = p.expected["terms"][0]
            ok["|l - x| <= 5"] = bool(np.abs(p.A @ p.B + p.bias - x).max() <= 5)
            ok["loss terms: multiples of 2^-5"] = bool((t * 32 == np.rint(t * 32)).all())
            # the largest tile's sum of absolute terms, in units of 2^-5, stays below 2^24: every partial sum inside a tile is exact.
            # (taken over 128 x 128 blocks padded up: a bound for every smaller tile too)
            Mp, Np = -(-p.M // 128) * 128, -(-p.N // 128) * 128
            tp = np.zeros((Mp, Np))
            tp[:p.M, :p.N] = np.abs(t)
            ok["tile loss sum < 2^24 units of 2^-5"] = bool(tile_sums(tp, 128, 128).max() * 32 < 2 ** 24)
            d = p.expected["out"][0]
            ok["gradient is exact in bf16"] = bool((bf16_round(d) == d).all())
    r32 = reference(p, np.float32)
    ok["float32 and float64 references agree bit for bit"] = all(
        np.array_equal(r32[k][0].view(np.uint64), p.expected[k][0].view(np.uint64)) for k in p.expected)
    return ok
