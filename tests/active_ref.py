"""TEST INFRASTRUCTURE: CPU restatements of the active-learning entries (include/bnn_hip.h F10) in numpy -- the total
order of bnn_acquire_topk as a lexsort, the whole launch's effect on the pool's state, the composed epoch order and the
random scores over the oracle's Philox restatement."""
import numpy as np

from oracle import bnn_oracle as O

COUNTER_WORDS = (3, 1)          # words 2 and 3 of the random scores' counter (row >> 2, round, 3, 1)


def rank_key(scores):
    """uint32 [N], ascending in the acquisition order: larger scores first, -0.0 equal to +0.0, every NaN last."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).copy()
    mag = u & np.uint32(0x7FFFFFFF)
    nan = mag > np.uint32(0x7F800000)
    u[mag == 0] = 0
    up = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))        # ascending with the score
    return np.where(nan, np.uint32(0xFFFFFFFF), ~up).astype(np.uint32)


def order(scores, candidate):
    """int32: every candidate row, best first -- (key ascending, row ascending) by lexsort."""
    rows = np.flatnonzero(np.asarray(candidate) != 0)
    key = rank_key(scores)[rows]
    return rows[np.lexsort((rows, key))].astype(np.int32)


def topk(scores, candidate, k, labelled, n_labelled):
    """(selected [k], candidate after, labelled after, n_labelled after, number selected) of one launch."""
    best = order(scores, candidate)
    m = min(int(k), best.size)
    selected = np.full(int(k), -1, np.int32)
    selected[:m] = best[:m]
    cand = np.array(candidate, dtype=np.uint8, copy=True)
    cand[best[:m]] = 0
    lab = np.array(labelled, dtype=np.int32, copy=True)
    lab[n_labelled:n_labelled + m] = best[:m]
    return selected, cand, lab, n_labelled + m, m


def compose(labelled, perm):
    """order[i] = labelled[perm[i]]"""
    return np.asarray(labelled, np.int32)[np.asarray(perm)]


def random_scores(seed, rnd, N):
    """float32 [N]: (w >> 8) 2^-24 with w = word (i & 3) of Philox4x32-R((i >> 2, round, 3, 1), seed)."""
    i = np.arange(N, dtype=np.uint32)
    r = np.stack(O.philox4x32(i >> 2, np.uint32(rnd), COUNTER_WORDS[0], COUNTER_WORDS[1], seed & 0xFFFFFFFF,
                              (seed >> 32) & 0xFFFFFFFF), axis=-1)
    w = r[np.arange(N), i & 3].astype(np.uint32)
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
