"""NumPy restatement of the binarisation rule of csrc/binarize.hip (the stream-8 row of the noise table of section 4),
on top of philox_oracle.py: exact integer words, the exact uniform grid, one float32 compare.  Imports nothing of the package.

    out[r][c] = (u < x[r][c]) ? 1 : 0,   u = (w >> 8) * 2^-24,   w = word (idx & 3) of block (idx >> 2) of stream 8 at (seed, step = counter),
    idx = (row_base + r) * n_cols + c    ("bernoulli");          out = x > 0.5f   ("threshold")."""
import numpy as np

import philox_oracle as P

STREAM = 8
FLAT_LIMIT = 1 << 58                     # flat indices below this: block indices below P.BLK_LIMIT = 2^56


def flat_index(row_base, n_rows, n_cols):
    """idx [n_rows][n_cols] as Python-int-exact uint64"""
    assert row_base >= 0 and (int(row_base) + int(n_rows)) * int(n_cols) < FLAT_LIMIT
    r = np.arange(int(row_base), int(row_base) + int(n_rows), dtype=np.uint64)[:, None]
    return r * np.uint64(n_cols) + np.arange(int(n_cols), dtype=np.uint64)[None, :]


def layout(row_base, n_rows, n_cols):
    """(block, word) of every element: what the noise table's row names"""
    idx = flat_index(row_base, n_rows, n_cols)
    return idx >> np.uint64(2), (idx & np.uint64(3)).astype(np.int64)


def words(seed, counter, row_base, n_rows, n_cols):
    """the 32-bit word of every element [n_rows][n_cols] (uint64 holding values < 2^32); each block of the call's flat range is computed once"""
    first = int(row_base) * int(n_cols)
    end = first + int(n_rows) * int(n_cols)
    assert row_base >= 0 and end < FLAT_LIMIT
    b0, b1 = first >> 2, (end - 1) >> 2
    w = P.block(seed, counter, STREAM, np.arange(b0, b1 + 1, dtype=np.uint64)).reshape(-1)
    return w[first - 4 * b0: end - 4 * b0].reshape(int(n_rows), int(n_cols))


def uniforms(seed, counter, row_base, n_rows, n_cols):
    """u as float32: (w >> 8) has 24 bits, so the product with 2^-24 is exact in float32"""
    return (words(seed, counter, row_base, n_rows, n_cols) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def binarize(X, seed=0, counter=0, row_base=0, mode="bernoulli"):
    """the rule on a float32 array X [n_rows][n_cols] -> float32 0 / 1; a NaN compares false"""
    X = np.asarray(X, dtype=np.float32)
    assert X.ndim == 2
    if mode == "threshold":
        return (X > np.float32(0.5)).astype(np.float32)
    assert mode == "bernoulli"
    with np.errstate(invalid="ignore"):
        return (uniforms(seed, counter, row_base, *X.shape) < X).astype(np.float32)
