"""Prints the constant of tests/test_gpu_binarize.py::test_frequency_of_the_draws_follows_x: for the fixed 4 x 64 input of values in (0, 1) below,
seed 0 and counters 0 .. 255, the largest |mean of the 256 draws - x| over the 256 elements as the ORACLE (binarize_oracle.py, on the CPU) draws
them.  The test's bound is twice this figure.  Run:  python tests/helpers/binarize_frequency_bound.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import binarize_oracle as BO      # noqa: E402

N_DRAWS = 256


def frequency_input():
    """4 x 64 distinct values (k + 0.5) / 256, k a fixed permutation of 0 .. 255: every value strictly inside (0, 1), exact in float32"""
    k = (np.arange(256, dtype=np.int64) * 37 + 11) % 256
    return ((k.astype(np.float32) + np.float32(0.5)) / np.float32(256.0)).reshape(4, 64)


def max_deviation(draw):
    """max over the elements of |mean_c draw(counter c) - x|, c = 0 .. N_DRAWS - 1; draw(X, counter) -> 0 / 1 array like X"""
    X = frequency_input()
    mean = np.zeros(X.shape, np.float64)
    for c in range(N_DRAWS):
        mean += np.asarray(draw(X, c), dtype=np.float64)
    return float(np.abs(mean / N_DRAWS - X.astype(np.float64)).max())


if __name__ == "__main__":
    d = max_deviation(lambda X, c: BO.binarize(X, seed=0, counter=c))
    print("oracle max |mean - x| = %.10f   bound (2 x) = %.10f" % (d, 2.0 * d))
