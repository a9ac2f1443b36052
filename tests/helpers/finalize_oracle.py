"""A float32 model of step_finalize_block (csrc/common.h) that reproduces the device's ORDER of additions, the inputs its tests use and
their case table (tests/test_gpu_step_finalize.py; the model is checked on the CPU by tests/test_finalize_host.py).  No GPU, no library here.

Block 0 (256 threads): thread t adds rp[t], rp[t + 256], ... ascending from 0.f (likewise the even and the odd entries of lp); wave_sum
is the xor butterfly v = v + v[lane ^ o], o = 32 .. 1; the four wave sums are joined as (red0 + red1) + (red2 + red3); one multiply by
inv_B gives recon, klz and klc.  loss = recon + kl_ratio * (klc + klz) and epoch_x += x * epoch_weight: every multiply there -- the
three by inv_B included -- feeds an add, and a compiler free to contract them into fused multiply-adds picks among a dozen roundings
(hipcc made fl(csum * inv_B + klz) and fl(rsum * inv_B + fl(kl_ratio * t)) of the first line: `loss_patterns`, SHIPPED_BEFORE).  The
kernel compiles block 0 under `#pragma clang fp contract(off)`: one rounding per operator, so every field has ONE value here.  The
contracted forms are still computed, exactly (fractions.Fraction, rounded to float32 once: no double rounding through float64), so that
the host test can require inputs on which they differ from the accepted value and a failing GPU test can name the form it met.
Blocks 1..: thread (rg, col) adds rows rg, rg + 16, ... of its column ascending from 0.f, then the 16 group sums are added ascending
from 0.f.  State: noise_step + 1; cursor (c + 1) % bpe, 0 when bpe == 0; with bump_adam adam_t + 1 and lr_t = lr_t(adam_t + 1), else both
untouched.

order = "model" is the device's; "descending" (every thread's chain and the join of the row groups backwards), "pairing" (the wave sums joined as (0 + 2) + (1 + 3)) and
"pairwise" (np.sum) are wrong orders the host test tells apart from it on the test inputs."""
import collections
import fractions

import numpy as np

import adam_exact as AX
import gemm_exact as GX

F = np.float32
OFF, ON = "off", "on"                                   # FMA contraction of a multiply feeding an add
ACCEPT = (OFF,)                                         # block 0 is compiled under contract(off): the uncontracted value alone
SHIPPED_BEFORE = ("klc", "recon")                       # the loss_patterns key of what hipcc (ROCm 7.2) made of the loss line without the pragma, in all five kernels
ORDERS = ("model", "descending", "pairing", "pairwise")

# (nr, nl, nblk, ncol)
CASES = ((1, 1, 1, 1), (3, 5, 1, 20), (255, 256, 16, 16), (256, 257, 17, 17), (300, 700, 37, 200), (1024, 512, 256, 1280), (1024, 512, 512, 1280))
KL_RATIO, EPOCH_WEIGHT, NOISE_STEP, LR_T_SENT, GOUT_GUARD = F(0.37), F(1.0 / 5.0), 41, F(-77.0), 64
ADAM_TS = (0, 7, 10 ** 6)
GOUT_SENT_BITS = 0x7FC12345
State = collections.namedtuple("State", "adam_t noise_step batch_cursor batches_per_epoch kl_ratio lr epoch_weight lr_t epoch_loss epoch_recon "
                                        "epoch_klz epoch_klc last_loss last_recon last_klz last_klc")
EPOCH_FIELDS = ("epoch_loss", "epoch_recon", "epoch_klz", "epoch_klc")
INEXACT_FIELDS = ("last_loss",) + EPOCH_FIELDS           # a multiply feeding an add


def case_id(c):
    return "nr%d-nl%d-nblk%d-ncol%d" % c


# ------------------------------------------------------------------------------------------------ exact rounding
def round_f32(x):
    """fractions.Fraction -> the nearest float32, ties to even, in one rounding"""
    x = fractions.Fraction(x)
    if x == 0:
        return F(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if fractions.Fraction(2) ** e > a:
        e -= 1
    assert fractions.Fraction(2) ** e <= a < fractions.Fraction(2) ** (e + 1)
    q = fractions.Fraction(2) ** (max(e, -126) - 23)    # the spacing of float32 at |x| (subnormals: 2^-149)
    n = a / q
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    r = lo * q
    assert r < fractions.Fraction(2) ** 128, "overflow"
    v = float(r)                                        # exact: at most 24 significant bits
    assert fractions.Fraction(v) == r
    return F(-v if x < 0 else v)


def fr(x):
    return fractions.Fraction(float(x))


def mul_add(a, b, c):
    """{OFF: fl(fl(a * b) + c), ON: fl(a * b + c)} in float32"""
    a, b, c = F(a), F(b), F(c)
    return {OFF: F(F(a * b) + c), ON: round_f32(fr(a) * fr(b) + fr(c))}


# ------------------------------------------------------------------------------------------------ block 0
def thread_sums(x, order="model"):
    """[256] float32: thread t's sum of x[t], x[t + 256], ... from 0.f (zero padding is exact: s + 0.f = s, and s is never -0.f)"""
    x = np.asarray(x, dtype=F)
    rows = max(1, -(-len(x) // 256))
    p = np.zeros(rows * 256, dtype=F)
    p[:len(x)] = x
    p = p.reshape(rows, 256)
    if order == "descending":
        p = p[::-1]
    acc = np.zeros(256, dtype=F)
    for r in p:
        acc = acc + r
    assert acc.dtype == F
    return acc


def wave_sum(v):
    """[.., 64] float32 -> the butterfly's result in every lane"""
    v = np.asarray(v, dtype=F)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    assert v.dtype == F
    return v


def block_sum_256(x, order="model"):
    if order == "pairwise":
        return F(np.sum(np.asarray(x, dtype=F), dtype=F))
    red = wave_sum(thread_sums(x, order).reshape(4, 64))[:, 0]
    if order == "pairing":
        return F(F(red[0] + red[2]) + F(red[1] + red[3]))
    return F(F(red[0] + red[1]) + F(red[2] + red[3]))


def block_sums(rp, lp, order="model"):
    """(rsum, zsum, csum): the three block sums before the multiply by inv_B"""
    lp = np.asarray(lp, dtype=F)
    return block_sum_256(rp, order), block_sum_256(lp[0::2], order), block_sum_256(lp[1::2], order)


def scalars(rp, lp, inv_B, order="model"):
    """(recon, klz, klc)"""
    inv_B = F(inv_B)
    return tuple(F(x * inv_B) for x in block_sums(rp, lp, order))


def loss_patterns(rsum, zsum, csum, inv_B, kl_ratio):
    """last_loss = recon + kl_ratio * (klc + klz) under every contraction of a multiply into the add it feeds: {(t, loss): value} with
    t = klc + klz as "off" fl(klc + klz) | "klc" fl(csum * inv_B + klz) | "klz" fl(klc + zsum * inv_B), and
    loss as "off" fl(recon + fl(kl_ratio * t)) | "kl" fl(recon + kl_ratio * t) | "recon" fl(rsum * inv_B + fl(kl_ratio * t))"""
    rsum, zsum, csum, inv_B, kl_ratio = (F(x) for x in (rsum, zsum, csum, inv_B, kl_ratio))
    recon, klz, klc = F(rsum * inv_B), F(zsum * inv_B), F(csum * inv_B)
    ts = {"off": F(klc + klz), "klc": round_f32(fr(csum) * fr(inv_B) + fr(klz)), "klz": round_f32(fr(klc) + fr(zsum) * fr(inv_B))}
    out = {}
    for tk, t in ts.items():
        P = F(kl_ratio * t)
        out[(tk, "off")] = F(recon + P)
        out[(tk, "kl")] = round_f32(fr(recon) + fr(kl_ratio) * fr(t))
        out[(tk, "recon")] = round_f32(fr(rsum) * fr(inv_B) + fr(P))
    return out


# ------------------------------------------------------------------------------------------------ blocks 1..
def column_sums(part, order="model"):
    """[nblk][ncol] -> [ncol]"""
    part = np.asarray(part, dtype=F)
    nblk, ncol = part.shape
    if order == "pairwise":
        return np.sum(np.ascontiguousarray(part.T), axis=1, dtype=F)      # (along the contiguous axis: NumPy's pairwise scheme)
    rows = max(1, -(-nblk // 16))
    p = np.zeros((rows * 16, ncol), dtype=F)
    p[:nblk] = part
    p = p.reshape(rows, 16, ncol)
    if order == "descending":
        p = p[::-1]
    acc = np.zeros((16, ncol), dtype=F)
    for r in p:
        acc = acc + r
    t = np.zeros(ncol, dtype=F)
    for g in (range(15, -1, -1) if order == "descending" else range(16)):
        t = t + acc[g]
    assert t.dtype == F
    return t


# ------------------------------------------------------------------------------------------------ the whole launch
Expected = collections.namedtuple("Expected", "exact gout contracted")


def finalize(rp, lp, inv_B, st, bump_adam, part, order="model", b1=AX.B1, b2=AX.B2):
    """Expected(exact = field -> the one value of every state field, gout, contracted = {"last_loss": loss_patterns, epoch field: its fused
    value}: what the kernel must NOT give where it differs from exact)"""
    rsum, zsum, csum = block_sums(rp, lp, order)
    inv_B = F(inv_B)
    recon, klz, klc = F(rsum * inv_B), F(zsum * inv_B), F(csum * inv_B)
    t = F(klc + klz)
    P = F(F(st.kl_ratio) * t)
    loss = F(recon + P)
    exact = {"last_loss": loss, "last_recon": recon, "last_klz": klz, "last_klc": klc, "noise_step": st.noise_step + 1, "batches_per_epoch": st.batches_per_epoch,
             "batch_cursor": (st.batch_cursor + 1) % st.batches_per_epoch if st.batches_per_epoch > 0 else 0,
             "kl_ratio": F(st.kl_ratio), "lr": F(st.lr), "epoch_weight": F(st.epoch_weight),
             "adam_t": st.adam_t + 1 if bump_adam else st.adam_t,
             "lr_t": AX.lr_t(st.adam_t + 1, F(st.lr), F(b1), F(b2)) if bump_adam else F(st.lr_t)}
    contracted = {"last_loss": loss_patterns(rsum, zsum, csum, inv_B, st.kl_ratio)}
    for name, x in (("epoch_loss", loss), ("epoch_recon", recon), ("epoch_klz", klz), ("epoch_klc", klc)):
        ma = mul_add(x, st.epoch_weight, getattr(st, name))
        exact[name] = ma[OFF]
        contracted[name] = ma[ON]
    assert bits(contracted["last_loss"][("off", "off")]) == bits(loss)
    return Expected(exact, column_sums(part, order), contracted)


def bits(x):
    return int(np.asarray(x, dtype=F).view(np.uint32))


def diagnose(exp, field, value):
    """a word on a value of an inexact field that is not the oracle's: the contracted form it has the bits of, if any"""
    if field == "last_loss":
        hit = [k for k, v in exp.contracted["last_loss"].items() if bits(v) == bits(value) and k != ("off", "off")]
        return "the contracted form(s) %r of recon + kl_ratio * (klc + klz)" % (hit,) if hit else "no contraction of the line gives it"
    if field in EPOCH_FIELDS:
        return "the fused multiply-add" if bits(exp.contracted[field]) == bits(value) else "not the fused multiply-add either (on the oracle's %s)" % field[6:]
    return ""


# ------------------------------------------------------------------------------------------------ inputs
Inputs = collections.namedtuple("Inputs", "rp lp part inv_B")


# seed of each case's inputs: the first for which every wrong order that CAN differ from the model's does, in at least one output, last_loss
# differs from the contracted form the kernels had before the pragma, and an epoch sum from its fused multiply-add (see `discriminates`)
# -- checked by the host test
SEEDS = {(1, 1, 1, 1): 57, (3, 5, 1, 20): 16, (255, 256, 16, 16): 19, (256, 257, 17, 17): 6, (300, 700, 37, 200): 69, (1024, 512, 256, 1280): 409,
         (1024, 512, 512, 1280): 1529}


def inputs(case, seed=None):
    """positive loss partials spanning a few decades, signed prior partials randn * 10 ** uniform(-3, 3): sums whose float32 value depends
    on the order of the additions"""
    nr, nl, nblk, ncol = case
    seed = SEEDS.get(tuple(case), 0) if seed is None else seed
    rng = np.random.RandomState(1000 * seed + 7 * nr + 5 * nl + 3 * nblk + ncol)
    rp = (rng.rand(nr) * 10 ** rng.uniform(0, 3, size=nr)).astype(F) + F(1e-3)
    lp = (rng.rand(2 * nl) * 10 ** rng.uniform(0, 3, size=2 * nl)).astype(F) + F(1e-3)
    part = (rng.randn(nblk, ncol) * 10 ** rng.uniform(-3, 3, size=(nblk, ncol))).astype(F)
    return Inputs(rp, lp, part, F(1.0 / 100.0))


def initial_state(adam_t, wrap):
    """non-trivial: the cursor at bpe - 1 (wraps to 0) or bpe = 0 with a stale cursor; non-zero epoch sums; lr_t a sentinel"""
    return State(adam_t=adam_t, noise_step=NOISE_STEP, batch_cursor=12 if wrap else 5, batches_per_epoch=13 if wrap else 0, kl_ratio=KL_RATIO, lr=AX.LR,
                 epoch_weight=EPOCH_WEIGHT, lr_t=LR_T_SENT, epoch_loss=F(12.625), epoch_recon=F(11.3125), epoch_klz=F(0.71875), epoch_klc=F(1.40625),
                 last_loss=F(-1.0), last_recon=F(-2.0), last_klz=F(-3.0), last_klc=F(-4.0))


def distinguishable(case, order):
    """can `order` differ from the model on this case at all?  A chain of two additions from 0.f is commutative, a lone value has no order:
    descending (every thread's chain AND the join of the 16 row groups backwards) needs three values in a chain (nr or nl > 512, three
    rows of partials); the pairing three waves with values (nr or nl > 128); np.sum three values anywhere"""
    nr, nl, nblk, ncol = case
    if order == "descending":
        return nr > 512 or nl > 512 or nblk >= 3
    if order == "pairing":
        return nr > 128 or nl > 128
    return nr >= 3 or nl >= 3 or nblk >= 3


def discriminates(case, seed=None):
    """what the inputs of `case` tell apart, as a dict of booleans (all must hold)"""
    inp = inputs(case, seed)
    st = initial_state(7, True)
    model = finalize(inp.rp, inp.lp, inp.inv_B, st, 1, inp.part)
    ok = {}
    for order in ORDERS[1:]:
        w = finalize(inp.rp, inp.lp, inp.inv_B, st, 1, inp.part, order)
        ds = any(bits(model.exact[k]) != bits(w.exact[k]) for k in ("last_recon", "last_klz", "last_klc"))
        dg = not np.array_equal(model.gout.view(np.uint32), w.gout.view(np.uint32))
        ok[order + ": an output differs"] = (ds or dg) if distinguishable(case, order) else not (ds or dg)
        if order == "pairing":
            ok["pairing: the column sums are the model's"] = not dg
    ok["last_loss differs from the contracted form compiled before the pragma"] = bits(model.exact["last_loss"]) != bits(model.contracted["last_loss"][SHIPPED_BEFORE])
    ok["an epoch sum differs from its fused multiply-add"] = any(bits(model.exact[k]) != bits(model.contracted[k]) for k in EPOCH_FIELDS)
    return ok


# ------------------------------------------------------------------------------------------------ the launches that carry riders
EINVAL = -1                                             # DMVAE_EINVAL (include/dmvae_hip.h)
FIN_14, FIN_2 = (300, 700, 37, 200), (255, 256, 16, 16)  # 1 + 13 blocks: lead 16;  1 + 1 blocks: lead 8, six idle ids
Carrier = collections.namedtuple("Carrier", "id pair M N K tile knobs bm bn nstage nw carries_fin")


def carriers():
    """the dense dX launches of gemm_bf16_dx_riders_kernel, each at the smallest shape with an interior tile, a last tile and more than one
    K tile.  dZ (LATENT, N = 64, K = 1024 = 16 K tiles): the 64-, 32- and 16-row tiles of knob 18 on M = 192 -- dmvae_gemm takes M in
    multiples of 64 only (the 32- and 16-row tiles would make three tiles of 96 and 48 rows; they make six and twelve of these); the
    16-row tile has two waves: 128-thread riders, and no step_finalize.  dX (RELU_MASK): every tile form on a 3 x 2 tile grid, K = 192
    (three K tiles; 128 on the two-slot ring of knob 7)"""
    out = [Carrier("dz-64rows", "dx_latent", 192, 64, 1024, (0, 0), {18: 0}, 64, 64, 4, 4, True),
           Carrier("dz-32rows", "dx_latent", 192, 64, 1024, (0, 0), {18: 1}, 32, 64, 4, 4, True),
           Carrier("dz-16rows", "dx_latent", 192, 64, 1024, (0, 0), {18: 2}, 16, 64, 4, 2, False)]
    for f in GX.FORMS.values():
        out.append(Carrier("dx-" + f.name, "dx_relu_mask", 3 * f.bm, 2 * f.bn, 128 if f.short else 192, (f.bm, f.bn), dict(f.knobs), f.bm, f.bn, f.nstage, f.nw, True))
    return out


# rider sets: (id, step_finalize case or None, gather: None | (ngat, gat_last, through the state's cursor))
RIDER_SETS = (("fin14", FIN_14, None), ("fin2", FIN_2, None), ("gat8-first", None, (8, 0, False)), ("gat24-last", None, (24, 1, False)),
              ("fin14+gat8-first", FIN_14, (8, 0, False)), ("fin2+gat24-last", FIN_2, (24, 1, False)), ("gat8-first-cursor", None, (8, 0, True)))
GATHER_DIMS = (20, 10)                                  # the 16-byte fast path | element loads
GATHER_N, GATHER_LD, GATHER_BPAD, GATHER_NVALID, GATHER_FIRST = 150, 64, 128, 100, 90      # rows 60 .. 99 of the batch lie past the data set: zeros
GATHER_CURSOR_BATCH = 7                                 # first = cursor * batch = 12 * 7 = 84 (initial_state(.., wrap=True))

# grouped heads' dX: (id, knobs, ((M, N, K), ..), profiler row)
STREAM_ROW, GROUPED_ROW = "heads_dx_stream_kernel", "gemm_bf16_grouped_mixed_tiles<L1, E3>"
_HEADS = (((192, 128, 64),), ((640, 384, 128), (640, 384, 128)), ((1024, 256, 256),))      # the streaming kernel's three bodies (K = 64 / 128 / 256)


def grouped_cases():
    out = []
    for shapes in _HEADS:
        tag = "%dx%dxK%s" % (shapes[0][0], shapes[0][1], "+".join(str(s[2]) for s in shapes))
        out.append(("stream-" + tag, {13: 1}, shapes, STREAM_ROW))
        for nw in (4, 8):
            out.append(("tiles-w%d-%s" % (nw, tag), {13: 0, 9: nw}, shapes, GROUPED_ROW))
    out.append(("declined-192x128xK512+64", {13: 1}, ((192, 128, 512), (192, 128, 64)), GROUPED_ROW))      # K = 512: streaming declines the group
    return out


def gemm_problem_keys():
    """every (pair, M, N, K) of gemm_exact these launches run: the host test checks that their references are exact"""
    keys = [(c.pair, c.M, c.N, c.K) for c in carriers()]
    for _, _, shapes, _ in grouped_cases():
        keys += [("dx_relu_mask",) + tuple(s) for s in shapes]
    return sorted(set(keys))


def gather_expected(data, perm, first, n_valid, B_pad, ld):
    """[B_pad][ld] float32: row r < n_valid = data[perm[first + r]] where first + r and the entry lie inside the data set, else zeros"""
    n, dim = data.shape
    out = np.zeros((B_pad, ld), dtype=F)
    for r in range(n_valid):
        s = first + r
        if 0 <= s < n and 0 <= perm[s] < n:
            out[r, :dim] = data[perm[s]]
    return out
