"""NumPy restatement of the device noise of csrc/common.h and of the counter layout of every kernel that draws from it -- the
"noise streams" table of DESIGN.md section 4, which is the contract; this file restates it and imports nothing of the package.

Philox4x32-10 is integer arithmetic: the words here are exact (tests/test_philox_host.py holds them against the Random123
known-answer vectors) and so is the uniform transform.  The normal and Gumbel transforms are evaluated in float64 from those words.

A block is one call of the cipher: four 32-bit words.  A SLOT names one of the values a block yields: word 0..3 for the uniform
and Gumbel transforms, normal 0..3 for the Box-Muller transform (words 0,1 -> normals 0,1; words 2,3 -> normals 2,3).
`philox_normal_at(idx)` of common.h is normal (idx & 1) of block (idx >> 1): it never uses words 2 and 3."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key schedule (Weyl) increments
MASK32 = np.uint64(0xFFFFFFFF)
STREAM_EPS, STREAM_GUMBEL, STREAM_EVAL, STREAM_GMM_SEED = 0, 1, 2, 3
BLK_LIMIT = 1 << 56                      # stream_id << 24 lands in bits 56..63 of the block index: blocks below this keep the streams apart
TWO_PI = 2.0 * np.pi


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(counter_words, k0, k1):
    """counter_words [..., 4] (values < 2^32), keys scalar or broadcastable to [...] -> uint64 array [..., 4] of 32-bit words"""
    c = _u64(counter_words)
    c0, c1, c2, c3 = (c[..., i] & MASK32 for i in range(4))
    k0 = _u64(k0) & MASK32
    k1 = _u64(k1) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1)


def block(seed, step, stream_id, blk):
    """philox_block: words of block `blk` (scalar or array of Python ints / uint64) of stream (seed, step, stream_id)"""
    blk = _u64(blk)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    ctr = np.empty(blk.shape + (4,), np.uint64)
    ctr[..., 0] = blk & MASK32
    ctr[..., 1] = (blk >> np.uint64(32)) ^ np.uint64((int(stream_id) << 24) & 0xFFFFFFFF)
    ctr[..., 2] = np.uint64(step & 0xFFFFFFFF)
    ctr[..., 3] = np.uint64(step >> 32)
    return philox4x32_10(ctr, seed & 0xFFFFFFFF, seed >> 32)


# ---------------------------------------------------------------------------------------------- transforms (float64, from the words)
def uniform(w):
    """[0, 1) on the 2^-24 grid (philox_uniform_at): exactly representable in float32"""
    return (_u64(w) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def u01(w):
    """(0, 1] on the 2^-24 grid (u01 of common.h): exactly representable in float32"""
    return ((_u64(w) >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def normal4(words):
    """words [..., 4] -> the block's four normals [..., 4]"""
    words = _u64(words)
    out = np.empty(words.shape, np.float64)
    for p in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u01(words[..., p])))
        ang = TWO_PI * u01(words[..., p + 1])
        out[..., p], out[..., p + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out


def gumbel(w):
    """-log(1e-20f - log(U)), U = u01(w).  The float32 sum 1e-20f - log(U) is -log(U) unless log(U) == 0 (U = 1): there it is 1e-20f."""
    l = np.log(u01(w))
    return -np.log(np.where(l == 0.0, np.float64(np.float32(1e-20)), -l))


# ---------------------------------------------------------------------------------------------- element streams (the C ABI's three launches)
def words_flat(seed, step, stream_id, n, first_block=0):
    """words 0 .. n-1 of the stream counted from block `first_block`: word i = word (i & 3) of block first_block + (i >> 2)"""
    nb = (int(n) + 3) // 4
    return block(seed, step, stream_id, np.arange(first_block, first_block + nb, dtype=np.uint64)).reshape(-1)[:n]


def uniform_at(seed, step, stream_id, idx):
    idx = _u64(idx)
    w = block(seed, step, stream_id, idx >> np.uint64(2))
    return uniform(np.take_along_axis(w, (idx & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0])


def gumbel_at(seed, step, stream_id, idx):
    idx = _u64(idx)
    w = block(seed, step, stream_id, idx >> np.uint64(2))
    return gumbel(np.take_along_axis(w, (idx & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0])


def normal_at(seed, step, stream_id, idx):
    idx = _u64(idx)
    n = normal4(block(seed, step, stream_id, idx >> np.uint64(1)))
    return np.take_along_axis(n, (idx & np.uint64(1)).astype(np.int64)[..., None], -1)[..., 0]


def normals_at(seed, step, stream_id, blk, slot):
    """normal `slot` of block `blk` (arrays of one shape): what a layout function's (block, slot) names"""
    n = normal4(block(seed, step, stream_id, blk))
    return np.take_along_axis(n, np.asarray(slot, np.int64)[..., None], -1)[..., 0]


# ---------------------------------------------------------------------------------------------- counter layouts, one per consumer
def _grid(B, D):
    b, d = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(D, dtype=np.uint64), indexing="ij")
    return b, d


def latent_lds_bytes(K, RB, dc):
    """latent_body.h latent_lds_bytes: tables 2 K (dc + 1) | c_k K | weights, softmax, sk 3 RB K | rows 2 RB (dc + 1) | RB | 32 floats"""
    return 4 * (2 * K * (dc + 1) + K + 3 * RB * K + 2 * RB * (dc + 1) + RB + 32)


def one_kernel_geometry(B_pad, D, K, blocks_target=512):
    """latent.hip latent_geometry: (RB rows per block, DC columns per chunk, nchunks, DSL columns per lane and chunk).  The chunk
    width follows from D, and from K and the rows per block through the 60 KiB LDS budget -- so the key of a column depends on them."""
    want = (B_pad + blocks_target - 1) // blocks_target
    RB = 16
    while RB < want and RB < 64:
        RB *= 2
    DC = 256
    while DC > 16 and DC // 2 >= D:
        DC //= 2
    while DC > 16 and latent_lds_bytes(K, RB, DC) > 60 * 1024:
        DC //= 2
    return RB, DC, (D + DC - 1) // DC, DC // 16


def latent_one_kernel(B, D, K, B_pad=None, width=None):
    """latent_body.h (latent_fwd_kernel, and heads_latent_kernel, which runs 16-row blocks of at most 4096 rows: the same geometry):
    column d lies in chunk c = d / DC at local column l = d % DC, which lane l & 15 of the row's sixteen holds as its column i = l >> 4;
    one block per four of a lane's columns: block (((b * nchunks + c) * 16 + lane) * ceil(DSL / 4)) + (i >> 2), normal i & 3.
    width: columns to lay out (default D; nchunks * DC = everything the lanes draw, padding columns included)"""
    B_pad = B_pad or (B + 63) // 64 * 64
    _, DC, nchunks, DSL = one_kernel_geometry(B_pad, D, K)
    b, d = _grid(B, D if width is None else width)
    c, l = d // np.uint64(DC), d % np.uint64(DC)
    lane, i = l & np.uint64(15), l >> np.uint64(4)
    G = np.uint64((DSL + 3) // 4)
    return ((b * np.uint64(nchunks) + c) * np.uint64(16) + lane) * G + (i >> np.uint64(2)), (i & np.uint64(3)).astype(np.int64)


def one_kernel_width(B_pad, D, K):
    _, DC, nchunks, _ = one_kernel_geometry(B_pad, D, K)
    return nchunks * DC


def latent_mfma(B, D, width=None):
    """latent_mfma.hip: columns in quads over D padded to 64: block b * (Dp / 4) + d / 4, normal d & 3"""
    Dp = (D + 63) // 64 * 64
    b, d = _grid(B, D if width is None else width)
    return b * np.uint64(Dp // 4) + (d >> np.uint64(2)), (d & np.uint64(3)).astype(np.int64)


def latent_vade(B, D):
    """latent_vade.hip: philox_normal_at(b * D + d)"""
    b, d = _grid(B, D)
    idx = b * np.uint64(D) + d
    return idx >> np.uint64(1), (idx & np.uint64(1)).astype(np.int64)


def eval_draws(draws, n_rows, D, first=0, n=None):
    """eval_clusters.hip: philox_normal_at(((j * n_rows + pos) * D + d)), pos = first + r the row's position in the data set -> [draws, n, D]"""
    n = n_rows - first if n is None else n
    j = np.arange(draws, dtype=np.uint64)[:, None, None]
    pos = np.arange(first, first + n, dtype=np.uint64)[None, :, None]
    d = np.arange(D, dtype=np.uint64)[None, None, :]
    idx = (j * np.uint64(n_rows) + pos) * np.uint64(D) + d
    return idx >> np.uint64(1), (idx & np.uint64(1)).astype(np.int64)


def gumbel_layout(B, K):
    """latent_body.h: philox_gumbel_at(b * K + k): word (b K + k) & 3 of block (b K + k) >> 2"""
    b, k = _grid(B, K)
    idx = b * np.uint64(K) + k
    return idx >> np.uint64(2), (idx & np.uint64(3)).astype(np.int64)


# ---------------------------------------------------------------------------------------------- what each consumer draws
def eps_one_kernel(seed, step, B, D, K, B_pad=None):
    return normals_at(seed, step, STREAM_EPS, *latent_one_kernel(B, D, K, B_pad))


def eps_mfma(seed, step, B, D):
    return normals_at(seed, step, STREAM_EPS, *latent_mfma(B, D))


def eps_vade(seed, step, B, D):
    return normals_at(seed, step, STREAM_EPS, *latent_vade(B, D))


def eps_eval(seed, counter, draws, n_rows, D, first=0, n=None):
    return normals_at(seed, counter, STREAM_EVAL, *eval_draws(draws, n_rows, D, first, n))


def gumbel_latent(seed, step, B, K):
    blk, slot = gumbel_layout(B, K)
    w = block(seed, step, STREAM_GUMBEL, blk)
    return gumbel(np.take_along_axis(w, slot[..., None], -1)[..., 0])


def find_edge_word(seed, step, stream_id, edge, max_blocks=1 << 24, words=(0, 1, 2, 3), chunk=1 << 21):
    """first flat word index (4 * block + word, over the given word positions) within the first max_blocks blocks whose word is
    >= 0xFFFFFF00 (edge "top": u01 = 1) or < 0x100 (edge "bottom": u01 = 2^-24); None if there is none"""
    sel = np.asarray(words)
    for b0 in range(0, max_blocks, chunk):
        w = block(seed, step, stream_id, np.arange(b0, min(b0 + chunk, max_blocks), dtype=np.uint64))[:, sel]
        hit = w >= np.uint64(0xFFFFFF00) if edge == "top" else w < np.uint64(0x100)
        if hit.any():
            r, c = np.argwhere(hit)[0]
            return 4 * (b0 + int(r)) + int(sel[c])
    return None
