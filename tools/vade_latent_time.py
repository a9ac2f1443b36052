"""Times the latent stage alone at large tables: VaDE's large-table form (dmvae_latent_fwd mode 2, csrc/latent_vade_mfma.hip) and DMVAE's MFMA
form (mode 0, csrc/latent_mfma.hip) at the same (rows, D, K), in one process.  Per kernel: the dispatch's own begin -> end timestamps (ProfScope,
dmvae_prof_collect kernel_ms) averaged over the launches; per stage: their sum, and the HIP-event time of the launches back to back.
    python tools/vade_latent_time.py [B D K ...]        (default: 8192 256 50 and 8192 512 256)"""
import ctypes as C, math, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))
from dmvae_hip import _lib, prof_enable, prof_collect
from dmvae_hip._lib import lib, check
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
WARM, REPS = 5, 30


def run(B, D, K, mode):
    ldD, ldK = (D + 63) // 64 * 64, (K + 63) // 64 * 64
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev); g.manual_seed(B + D + K)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    mv = torch.cat([rn(B, ldD) * 1.2, rn(B, ldD) * 0.5 - 0.2], 1).contiguous()
    lgd, eps = rn(B, ldK), rn(B, D)
    pm, plv = rn(K, D) * 2.0 / math.sqrt(D), rn(K, D) * 0.4 / math.sqrt(D)
    Zb = torch.zeros(B, ldD, dtype=torch.bfloat16, device=dev); Zf = z(B, ldD); w = z(B, ldK)
    gmu, glv, clv = z(B, ldD), z(B, ldD), z(B, ldD); dlg = torch.zeros(B, ldK, dtype=torch.bfloat16, device=dev)
    nblk = lib.dmvae_latent_nblocks_vade(B) if mode == 2 else lib.dmvae_latent_nblocks(B, D, K)
    nb = int(lib.dmvae_latent_ws_bytes(B, D, K, mode))
    assert nb > 0, "shape (%d, %d, %d) does not take the MFMA form in mode %d" % (B, D, K, mode)
    ws = torch.empty(nb // 4, device=dev)
    dpri, lp = z(2 * K * D), z(max(nblk, B // 16), 2)                    # the MFMA forms deliver ONE set of prior-gradient partials
    a = _lib.LatentArgs()
    a.B, a.B_pad, a.D, a.K, a.mode, a.act_dtype = B, B, D, K, mode, _lib.BF16
    a.kl_ratio, a.temperature, a.inv_B, a.seed = 1.0, 0.5, 1.0 / B, 7
    a.mean, a.ld_mean = mv.data_ptr(), 2 * ldD
    a.log_var, a.ld_log_var = mv.data_ptr() + 4 * ldD, 2 * ldD
    a.logits, a.ld_logits = lgd.data_ptr(), ldK
    a.eps, a.ld_eps = eps.data_ptr(), D
    a.prior_means, a.prior_log_vars = pm.data_ptr(), plv.data_ptr()
    a.Z_act, a.ld_Z, a.Z_f32, a.ld_Zf = Zb.data_ptr(), ldD, Zf.data_ptr(), ldD
    a.weights, a.ld_w = w.data_ptr(), ldK
    a.gmu, a.glv, a.clv, a.ld_g = gmu.data_ptr(), glv.data_ptr(), clv.data_ptr(), ldD
    a.dlogits_act, a.ld_dl = dlg.data_ptr(), ldK
    a.dprior_partials, a.loss_partials = dpri.data_ptr(), lp.data_ptr()
    a.mfma_ws, a.mfma_ws_bytes = ws.data_ptr(), nb
    for _ in range(WARM): check(lib.dmvae_latent_fwd(st, C.byref(a)), "dmvae_latent_fwd")
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPS): lib.dmvae_latent_fwd(st, C.byref(a))
    t1.record(); torch.cuda.synchronize()
    wall = t0.elapsed_time(t1) / REPS * 1e3
    prof_enable(True)
    for _ in range(REPS): lib.dmvae_latent_fwd(st, C.byref(a))
    torch.cuda.synchronize()
    rows = prof_collect()
    prof_enable(False)
    assert torch.isfinite(lp).all() and torch.isfinite(gmu).all()
    name = "VaDE large-table (mode 2)" if mode == 2 else "DMVAE MFMA (mode 0)"
    total = sum(r["kernel_ms"] for r in rows) / REPS * 1e3
    print("B=%d D=%d K=%d %-26s scratch %6.1f MB | kernels %8.1f us | back to back %8.1f us" % (B, D, K, name, nb / 1e6, total, wall), flush=True)
    for r in rows:
        print("      %-22s %2d dispatches  %8.1f us" % (r["name"], r["kernel_launches"] // REPS, r["kernel_ms"] / REPS * 1e3), flush=True)
    return total


if __name__ == "__main__":
    v = [int(x) for x in sys.argv[1:]] or [8192, 256, 50, 8192, 512, 256]
    for i in range(0, len(v), 3):
        B, D, K = v[i:i + 3]
        tv, td = run(B, D, K, 2), run(B, D, K, 0)
        print("B=%d D=%d K=%d VaDE / DMVAE = %.2f" % (B, D, K, tv / td), flush=True)
