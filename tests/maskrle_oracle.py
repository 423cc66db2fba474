"""Numpy oracle of the run-length encoder (include/maskrle.h): the COCO run lengths of a binary mask and their inverse.  No
reference code in it; tests/test_maskrle_cpu.py checks the two against each other and against hand-written cases."""
import numpy as np


def runs_of(bits):
    """bits [H, W] (bool or 0/1) -> the counts as a list of Python ints: the mask walked in column-major order, the lengths of
    the alternating runs of equal bits, the first a run of zeros (0 when pixel (0, 0) is set)."""
    walk = np.asarray(bits).astype(np.int8).T.reshape(-1)
    change = np.flatnonzero(np.diff(walk, prepend=np.int8(0)))            # positions that differ from their predecessor
    edges = np.concatenate([[0], change, [walk.size]])
    return [int(c) for c in np.diff(edges)]


def decode(counts, H, W):
    """The inverse: counts -> bool [H, W]."""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() == H * W and (counts[1:] > 0).all() and counts[0] >= 0
    pattern = np.arange(len(counts)) % 2 == 1
    return np.repeat(pattern, counts).reshape(W, H).T
