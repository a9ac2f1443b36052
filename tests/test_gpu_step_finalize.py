"""step_finalize_block and gather_rows_block in every kernel they are compiled into, each held to an exact reference.

step_finalize_block (csrc/common.h) ends the forward pass of every training step: block 0 turns the loss partials into last_* / epoch_*,
advances adam_t / lr_t / noise_step and the batch cursor, blocks 1.. add the prior-table gradient partials in a fixed order.  It lives
in five kernels -- its own, the dense dX GEMM that carries riders (LATENT = the dZ GEMM, RELU_MASK = a layer's dX), the grouped dX tiles
and the streaming dX of the head layers -- and the step picks one by shape, dtype and knobs (csrc/step.hip place_riders).
gather_rows_block (csrc/gemm_epilogue.h) likewise runs in its own kernel (four quads per thread) and as a rider (sixteen, on 128, 256
or 512 threads, in the first or the last ids of the grid).  The entries of include/dmvae_hip_debug.h reach every home on buffers of
the test's: the stand-alone kernel against the float32 oracle of tests/helpers/finalize_oracle.py (the device's order of additions:
bit for bit, block 0's multiply-adds uncontracted); every carrier with riders against the same carrier without
(the public entry), against the exact integer product of tests/helpers/gemm_exact.py, and its riders against the stand-alone kernels,
bit for bit -- the GEMM's tile ids are shifted by the riders' ids, so a mapping fault drops one tile and computes another twice.
Sentinel guard bands around every output; the profiler rows name the instantiation that ran."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import adam_exact as AX            # noqa: E402
import finalize_oracle as FO       # noqa: E402
import gemm_exact as GX            # noqa: E402
from gemm_harness import bf16_name, collect, forced, kernels_launched, launched, setup, stream, verify             # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def hip():
    import dmvae_hip      # noqa: F401
    from dmvae_hip import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert _lib.lib.dmvae_debug_step_finalize and FO.EINVAL == -1
    return _lib


# ------------------------------------------------------------------------------------------------ step_finalize on buffers of the test's
def state_bytes(L, st):
    s = L.State()
    for k, v in st._asdict().items():
        setattr(s, k, v.item() if isinstance(v, np.generic) else v)
    return bytes(s)


def read_state(L, dev):
    """field -> value of a device dmvae_state (floats as np.float32: their bits are what is compared)"""
    s = L.State.from_buffer_copy(bytes(dev.cpu().numpy().tobytes()))
    return {k: (F(getattr(s, k)) if t is C.c_float else int(getattr(s, k))) for k, t in L.State._fields_}


class Fin:
    """the inputs of one step_finalize case on the device, and per launch a fresh state and a fresh gout between two guard bands"""

    def __init__(self, L, case):
        self.L, self.case = L, case
        self.nr, self.nl, self.nblk, self.ncol = case
        self.inp = FO.inputs(case)
        self.rp, self.lp, self.part = (torch.as_tensor(a).cuda() for a in (self.inp.rp, self.inp.lp, self.inp.part))

    def arm(self, st, bump):
        """-> (dmvae_debug_finalize, state tensor, gout tensor with its guards)"""
        L = self.L
        state = torch.frombuffer(bytearray(state_bytes(L, st)), dtype=torch.uint8).cuda()
        gout = torch.full((2 * FO.GOUT_GUARD + self.ncol,), FO.GOUT_SENT_BITS, dtype=torch.int32, device="cuda")
        f = L.DebugFinalize()
        f.rp, f.nr, f.lp, f.nl = self.rp.data_ptr(), self.nr, self.lp.data_ptr(), self.nl
        f.inv_B, f.state, f.bump_adam, f.b1, f.b2 = float(self.inp.inv_B), state.data_ptr(), bump, float(AX.B1), float(AX.B2)
        f.part, f.nblk, f.ncol, f.gout = self.part.data_ptr(), self.nblk, self.ncol, gout.data_ptr() + 4 * FO.GOUT_GUARD
        return f, state, gout

    def check(self, st, bump, state, gout, what):
        """outputs and every state field against the oracle, bit for bit"""
        exp = FO.finalize(self.inp.rp, self.inp.lp, self.inp.inv_B, st, bump, self.inp.part)
        g = gout.cpu().numpy()
        G = FO.GOUT_GUARD
        assert (g[:G] == FO.GOUT_SENT_BITS).all() and (g[G + self.ncol:] == FO.GOUT_SENT_BITS).all(), "%s: gout's guard bands were written" % what
        bad = np.nonzero(g[G:G + self.ncol].view(np.uint32) != exp.gout.view(np.uint32))[0]
        assert bad.size == 0, "%s: %d of %d prior-table sums are not the oracle's bits (first: column %d)" % (what, bad.size, self.ncol, bad[0])
        got = read_state(self.L, state)
        assert set(got) == set(exp.exact)
        for k, want in exp.exact.items():
            if isinstance(want, np.floating):
                assert FO.bits(got[k]) == FO.bits(want), "%s: %s = %r, the oracle has %r: %s" % (what, k, got[k], want, FO.diagnose(exp, k, got[k]))
            else:
                assert got[k] == want, "%s: %s = %r, the oracle has %r" % (what, k, got[k], want)


@pytest.mark.parametrize("case", FO.CASES, ids=FO.case_id)
def test_stand_alone_kernel_has_the_oracles_bits(hip, case):
    """step_finalize_kernel from a non-trivial state -- adam_t 0 / 7 / 10^6, the cursor wrapping at the end of an epoch and bpe = 0, both
    values of bump_adam, lr_t a sentinel, non-zero epoch sums: every output and every state field bit for bit, gout's guards intact"""
    L = hip
    fin = Fin(L, case)
    first = True
    for adam_t in FO.ADAM_TS:
        for wrap in (True, False):
            for bump in (1, 0):
                st = FO.initial_state(adam_t, wrap)
                f, state, gout = fin.arm(st, bump)
                what = "step_finalize %s adam_t=%d wrap=%d bump=%d" % (FO.case_id(case), adam_t, wrap, bump)
                if first:
                    names, _ = kernels_launched(L, lambda: launched(L, L.lib.dmvae_debug_step_finalize(stream(), C.byref(f)), what))
                    assert names == ["step_finalize"], names
                    first = False
                else:
                    launched(L, L.lib.dmvae_debug_step_finalize(stream(), C.byref(f)), what)
                fin.check(st, bump, state, gout, what)


def test_finalize_arguments_are_checked(hip):
    L = hip
    fin = Fin(L, FO.FIN_2)
    f, state, gout = fin.arm(FO.initial_state(7, True), 1)
    before = state.clone()
    for field in ("rp", "lp", "state", "part", "gout"):
        g = L.DebugFinalize.from_buffer_copy(bytes(f))
        setattr(g, field, None)
        assert L.lib.dmvae_debug_step_finalize(stream(), C.byref(g)) == FO.EINVAL, field
    g = L.DebugFinalize.from_buffer_copy(bytes(f))
    g.nblk = -1
    assert L.lib.dmvae_debug_step_finalize(stream(), C.byref(g)) == FO.EINVAL
    assert L.lib.dmvae_debug_step_finalize(stream(), None) == FO.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(state, before)


# ------------------------------------------------------------------------------------------------ the gather on buffers of the test's
class Gather:
    """a data set of GATHER_N rows of `dim` columns, a permutation, and per launch a fresh bf16 output [B_pad][ld] between two guard bands"""

    def __init__(self, L, dim, seed):
        self.L, self.dim = L, dim
        rng = np.random.RandomState(seed)
        self.data = rng.rand(FO.GATHER_N, dim).astype(F)
        self.perm = rng.permutation(FO.GATHER_N).astype(np.int32)
        self.d_data, self.d_perm = torch.as_tensor(self.data).cuda(), torch.as_tensor(self.perm).cuda()
        assert self.d_data.data_ptr() % 16 == 0

    def out(self):
        return torch.full((2 * GX.GUARD + FO.GATHER_BPAD * FO.GATHER_LD,), GX.SENT_BF16_BITS, dtype=torch.int16, device="cuda")

    def arm(self, first, batch, state):
        L = self.L
        o = self.out()
        g = L.DebugGather()
        g.data, g.n_rows, g.dim, g.perm, g.first = self.d_data.data_ptr(), FO.GATHER_N, self.dim, self.d_perm.data_ptr(), first
        g.batch, g.n_valid, g.B_pad = batch, FO.GATHER_NVALID, FO.GATHER_BPAD
        g.out_bf16, g.ld, g.state = o.data_ptr() + 2 * GX.GUARD, FO.GATHER_LD, (state.data_ptr() if state is not None else None)
        return g, o

    def stand_alone(self, first, batch, state):
        """dmvae_gather_rows with the same arguments"""
        L = self.L
        o = self.out()
        launched(L, L.lib.dmvae_gather_rows(stream(), L.BF16, L.ptr(self.d_data), FO.GATHER_N, self.dim, L.ptr(self.d_perm), first, batch, FO.GATHER_NVALID,
                                            FO.GATHER_BPAD, C.c_void_p(o.data_ptr() + 2 * GX.GUARD), FO.GATHER_LD, None, FO.GATHER_LD,
                                            L.ptr(state) if state is not None else None), "dmvae_gather_rows dim=%d" % self.dim)
        return o

    def check(self, o, first, what):
        h = o.cpu()
        assert bool((h[:GX.GUARD] == GX.SENT_BF16_BITS).all() and (h[-GX.GUARD:] == GX.SENT_BF16_BITS).all()), "%s: the gather wrote outside its output" % what
        want = torch.as_tensor(FO.gather_expected(self.data, self.perm, first, FO.GATHER_NVALID, FO.GATHER_BPAD, FO.GATHER_LD)).bfloat16().view(torch.int16)
        got = h[GX.GUARD:-GX.GUARD].view(FO.GATHER_BPAD, FO.GATHER_LD)
        assert torch.equal(got, want), "%s: %d elements of the gathered batch are wrong" % (what, int((got != want).sum()))
        assert bool((want[:FO.GATHER_N - first].view(torch.bfloat16).float().abs().sum(1) > 0).all()) and not bool(want[FO.GATHER_N - first:].any())


# ------------------------------------------------------------------------------------------------ riders of the dense dX launches
def _plain(L, c, p):
    """(a) the carrier without riders: dmvae_gemm"""
    b, e = setup(L, "bf16", p)
    what = "%s without riders" % c.id
    launched(L, L.lib.dmvae_gemm(stream(), L.BF16, GX.DX, p.M, p.N, p.K, C.c_void_p(b["A"].ptr), b["A"].ld, C.c_void_p(b["B"].ptr), b["B"].ld, C.byref(e), 1), what)
    return collect(b, what)


def _riders_call(L, p, b, e, f, g, ngat, gat_last):
    return L.lib.dmvae_debug_gemm_dx_riders(stream(), p.M, p.N, p.K, C.c_void_p(b["A"].ptr), b["A"].ld, C.c_void_p(b["B"].ptr), b["B"].ld, C.byref(e),
                                            C.byref(f) if f is not None else None, C.byref(g) if g is not None else None, ngat, gat_last)


@pytest.mark.parametrize("c", FO.carriers(), ids=lambda c: c.id)
def test_dense_dx_with_riders(hip, c):
    """(a) the carrier alone, (b) with every rider set, (c) the riders' stand-alone kernels: the GEMM output of (b) has the bits of (a) and
    is the exact product, finalize outputs and state of (b) are (c)'s byte for byte, the gathered batch of (b) is (c)'s and the expected
    rows; on the two-wave 16-row tile the finalize blocks are refused and the gather runs on 128 threads"""
    L = hip
    p = GX.make(c.pair, c.M, c.N, c.K)
    pair = GX.PAIRS[c.pair]
    want_name = bf16_name(c.bm, c.bn, pair, c.nstage, c.nw)
    fins = {case: Fin(L, case) for case in (FO.FIN_14, FO.FIN_2)}
    gathers = {dim: Gather(L, dim, seed=11 + dim) for dim in FO.GATHER_DIMS}
    st0 = FO.initial_state(7, True)
    with forced(L, c.tile, c.knobs):
        names, plain = kernels_launched(L, lambda: _plain(L, c, p))
        assert names == [want_name], (c.id, names)
        verify(p, "bf16", plain, 64, 64)
        profiled = False
        for sid, fcase, gat in FO.RIDER_SETS:
            for dim in (FO.GATHER_DIMS if gat else (None,)):
                what = "%s + %s%s" % (c.id, sid, "" if dim is None else " dim=%d" % dim)
                b, e = setup(L, "bf16", p)
                f = state = gout = g = gout_o = gstate = None
                if fcase:
                    f, state, gout = fins[fcase].arm(st0, 1)
                ngat = gat_last = 0
                first = FO.GATHER_FIRST
                if gat:
                    ngat, gat_last, cursor = gat
                    if cursor:
                        gstate = torch.frombuffer(bytearray(state_bytes(L, st0)), dtype=torch.uint8).cuda()
                        first = st0.batch_cursor * FO.GATHER_CURSOR_BATCH
                        g, gout_o = gathers[dim].arm(-12345, FO.GATHER_CURSOR_BATCH, gstate)
                    else:
                        g, gout_o = gathers[dim].arm(first, FO.GATHER_NVALID, None)
                if fcase and not c.carries_fin:
                    assert _riders_call(L, p, b, e, f, g, ngat, gat_last) == FO.EINVAL, what
                    torch.cuda.synchronize()
                    assert bool(collect(b, what)["out"][0].eq(GX.SENT_BF16_BITS).all()), "%s: refused, yet something ran" % what
                    continue
                if not profiled:
                    names, _ = kernels_launched(L, lambda: launched(L, _riders_call(L, p, b, e, f, g, ngat, gat_last), what))
                    assert names == [want_name], (what, names)
                    print("KERNEL %s -> %s" % (what, names[0]))
                    profiled = True
                else:
                    launched(L, _riders_call(L, p, b, e, f, g, ngat, gat_last), what)
                res = collect(b, what)
                assert torch.equal(res["out"][0], plain["out"][0]), "%s: %d elements of the GEMM output differ from the launch without riders" % (
                    what, int((res["out"][0] != plain["out"][0]).sum()))
                verify(p, "bf16", res, 64, 64)
                if fcase:
                    f2, state2, gout2 = fins[fcase].arm(st0, 1)
                    launched(L, L.lib.dmvae_debug_step_finalize(stream(), C.byref(f2)), what + ": stand-alone finalize")
                    fins[fcase].check(st0, 1, state2, gout2, what + ": stand-alone finalize")
                    assert torch.equal(gout, gout2), "%s: the prior-table sums differ from the stand-alone kernel's" % what
                    a_, b_ = read_state(L, state), read_state(L, state2)
                    diff = {k: (a_[k], b_[k]) for k in a_ if (FO.bits(a_[k]) != FO.bits(b_[k]) if isinstance(a_[k], np.floating) else a_[k] != b_[k])}
                    assert torch.equal(state, state2), "%s: state fields differ from the stand-alone kernel's: %r" % (what, diff)
                if gat:
                    if gstate is not None:
                        assert bytes(gstate.cpu().numpy().tobytes()) == state_bytes(L, st0), "%s: a gather wrote the state" % what
                    gathers[dim].check(gout_o, first, what)
                    alone = gathers[dim].stand_alone(-12345 if gstate is not None else first, FO.GATHER_CURSOR_BATCH if gstate is not None else FO.GATHER_NVALID, gstate)
                    assert torch.equal(gout_o, alone), "%s: the gathered batch differs from dmvae_gather_rows'" % what


def test_rider_launch_refusals(hip):
    """ngat not a multiple of 8; more riders than the launch has room for; step_finalize with a gather addressed through the state's cursor;
    no riders at all; another epilogue: DMVAE_EINVAL, nothing launched"""
    L = hip
    c = FO.carriers()[0]
    p = GX.make(c.pair, c.M, c.N, c.K)
    fin, gat = Fin(L, FO.FIN_2), Gather(L, 20, seed=3)
    st0 = FO.initial_state(7, True)
    with forced(L, c.tile, c.knobs):
        b, e = setup(L, "bf16", p)
        f, state, gout = fin.arm(st0, 1)
        gstate = torch.frombuffer(bytearray(state_bytes(L, st0)), dtype=torch.uint8).cuda()
        g, go = gat.arm(FO.GATHER_FIRST, FO.GATHER_NVALID, None)
        gs, gso = gat.arm(0, FO.GATHER_CURSOR_BATCH, gstate)
        assert _riders_call(L, p, b, e, None, g, 12, 0) == FO.EINVAL                 # ngat % 8
        assert _riders_call(L, p, b, e, None, g, 0, 0) == FO.EINVAL
        assert _riders_call(L, p, b, e, None, None, 0, 0) == FO.EINVAL               # no riders
        assert _riders_call(L, p, b, e, f, None, 8, 0) == FO.EINVAL                  # ngat without a gather
        assert _riders_call(L, p, b, e, f, gs, 8, 0) == FO.EINVAL                    # finalize moves the cursor the gather reads
        assert _riders_call(L, p, b, e, None, g, 512, 1) == FO.EINVAL                # 3 tiles + 512 > 512
        assert _riders_call(L, p, b, e, f, g, 504, 1) == FO.EINVAL                   # 3 + 8 + 504
        e2 = L.Epilogue.from_buffer_copy(bytes(e))
        e2.kind = GX.EPI_STORE_F32
        assert _riders_call(L, p, b, e2, f, None, 0, 0) == FO.EINVAL
        torch.cuda.synchronize()
        assert bool(collect(b, "refused")["out"][0].eq(GX.SENT_BF16_BITS).all())
        assert bytes(state.cpu().numpy().tobytes()) == state_bytes(L, st0) and bool((gout == FO.GOUT_SENT_BITS).all())
        assert bool((go == GX.SENT_BF16_BITS).all()) and bool((gso == GX.SENT_BF16_BITS).all())


# ------------------------------------------------------------------------------------------------ the grouped heads' dX with step_finalize riding
def _grouped(L, shapes, f):
    n = len(shapes)
    probs = (L.GemmProblem * n)()
    keep = []
    for i, (M, N, K) in enumerate(shapes):
        p = GX.make("dx_relu_mask", M, N, K)
        b, e = setup(L, "bf16", p)
        q = probs[i]
        q.M, q.N, q.K = M, N, K
        q.A, q.lda, q.B, q.ldb = b["A"].ptr, b["A"].ld, b["B"].ptr, b["B"].ld
        q.epi = e
        keep.append((p, b))
    if f is None:
        launched(L, L.lib.dmvae_gemm_grouped(stream(), L.BF16, GX.DX, probs, n), "dmvae_gemm_grouped")
    else:
        launched(L, L.lib.dmvae_debug_gemm_grouped_fin(stream(), probs, n, C.byref(f)), "dmvae_debug_gemm_grouped_fin")
    return [(p, collect(b, "grouped dX %dx%dx%d" % (p.M, p.N, p.K))) for p, b in keep]


@pytest.mark.parametrize("case", FO.grouped_cases(), ids=lambda g: g[0])
def test_grouped_dx_with_finalize(hip, case):
    """the heads' dX on the streaming kernel (its three bodies), on the grouped tiles with four and eight waves, and a group the streaming
    kernel declines: with 14 and with 2 finalize blocks in the first ids, every problem's output has the bits of the launch without them
    and is the exact product; finalize outputs and state are the stand-alone kernel's"""
    L = hip
    gid, knobs, shapes, row = case
    st0 = FO.initial_state(10 ** 6, False)
    with forced(L, (0, 0), knobs):
        names, plain = kernels_launched(L, lambda: _grouped(L, shapes, None))
        assert names == [row], (gid, names)
        for p, res in plain:
            verify(p, "bf16", res, 64, 64)
        for i, fcase in enumerate((FO.FIN_14, FO.FIN_2)):
            fin = Fin(L, fcase)
            what = "%s + %d finalize blocks" % (gid, 1 + -(-fcase[3] // 16))
            f, state, gout = fin.arm(st0, 1)
            if i == 0:
                names, out = kernels_launched(L, lambda: _grouped(L, shapes, f))
                assert names == [row], (what, names)
                print("KERNEL %s -> %s" % (what, names[0]))
            else:
                out = _grouped(L, shapes, f)
            for (p, res), (_, res0) in zip(out, plain):
                assert torch.equal(res["out"][0], res0["out"][0]), "%s: %d elements of %dx%dx%d differ from the launch without riders" % (
                    what, int((res["out"][0] != res0["out"][0]).sum()), p.M, p.N, p.K)
                verify(p, "bf16", res, 64, 64)
            f2, state2, gout2 = fin.arm(st0, 1)
            launched(L, L.lib.dmvae_debug_step_finalize(stream(), C.byref(f2)), what + ": stand-alone finalize")
            fin.check(st0, 1, state2, gout2, what + ": stand-alone finalize")
            assert torch.equal(gout, gout2), "%s: the prior-table sums differ from the stand-alone kernel's" % what
            a_, b_ = read_state(L, state), read_state(L, state2)
            diff = {k: (a_[k], b_[k]) for k in a_ if (FO.bits(a_[k]) != FO.bits(b_[k]) if isinstance(a_[k], np.floating) else a_[k] != b_[k])}
            assert torch.equal(state, state2), "%s: state fields differ from the stand-alone kernel's: %r" % (what, diff)
