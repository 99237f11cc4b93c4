"""TEST INFRASTRUCTURE: a numpy restatement of the BatchBALD entries (include/bnn_hip.h F15).  Phat, the exponents E, the
weights, the offsets and the sampled labels are restated in fp32 / integers / fp64 operation by operation and are meant to
be bit-equal to the device; the entropies are restated in fp64 from the same fp32 inputs.  Philox is the oracle's."""
import itertools

import numpy as np

from oracle import bnn_oracle as O

COUNTER_WORDS = (4, 1)          # words 2 and 3 of the label stream's counter (m, j | round << 8, 4, 1)
LN2 = float.fromhex("0x1.62e42fefa39efp-1")


def configs(C, n, max_configs):
    """Rows of Phat with n chosen rows: C^n while it does not exceed max_configs, else max_configs."""
    m = 1
    for _ in range(n):
        m *= C
        if m > max_configs:
            return max_configs
    return m


def is_exact(C, n, max_configs):
    return C ** n <= max_configs


class State:
    def __init__(self, phat, E, w, o, base):
        self.phat, self.E, self.w, self.o, self.base = phat, E, w, o, base

    @property
    def M(self):
        return self.phat.shape[0]


def begin(S):
    return State(np.ones((1, S), np.float32), np.zeros(1, np.int32), np.ones(1, np.float64), np.zeros(1, np.float64), np.float64(0.0))


def rescale(rows):
    """Every row times 2^-e, (f, e) = frexp(row max); e = 0 for an all-zero row.  Exact."""
    rows = np.asarray(rows, np.float32)
    mx = rows.max(axis=1)
    _, e = np.frexp(mx)
    e = np.where(mx > 0, e, 0).astype(np.int32)
    return np.ascontiguousarray(np.ldexp(rows, -e[:, None]), dtype=np.float32), e


def uniforms(seed, rnd, M, j):
    m = np.arange(M, dtype=np.uint32)
    c1 = np.uint32((j | (rnd << 8)) & 0xFFFFFFFF)
    w0 = O.philox4x32(m, c1, COUNTER_WORDS[0], COUNTER_WORDS[1], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (w0.astype(np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def labels(seed, rnd, j, prow):
    """Inverse-CDF labels of rows m = 0 .. M-1 from prow [M, C] = P[s_m, i_j, :]."""
    prow = np.asarray(prow, np.float32)
    M, C = prow.shape
    cum = np.cumsum(prow, axis=1, dtype=np.float32)                # sequential fp32 sums in ascending class order
    t = (uniforms(seed, rnd, M, j) * cum[:, -1]).astype(np.float32)
    return np.minimum((cum <= t[:, None]).sum(axis=1), C - 1).astype(np.int64)


def extend(st, P, cond, chosen, max_configs, seed=0, rnd=0):
    """The state after `chosen` (rows in the order chosen, the winner last) from the state before the winner."""
    S, N, C = P.shape
    n, i = len(chosen), chosen[-1]
    if is_exact(C, n, max_configs):
        rows = (st.phat[:, None, :] * P[:, i, :].T[None, :, :]).astype(np.float32).reshape(st.M * C, S)
        rows, e = rescale(rows)
        E = (np.repeat(st.E, C) + e).astype(np.int32)
        w = np.ldexp(np.float64(1.0), E).astype(np.float64)
    else:
        M = max_configs
        sm = np.arange(M) % S
        if is_exact(C, n - 1, max_configs):
            rows, E, j0 = np.ones((M, S), np.float32), np.zeros(M, np.int32), 0
        else:
            rows, E, j0 = st.phat.copy(), st.E.copy(), n - 1
        for j in range(j0, n):
            ij = chosen[j]
            y = labels(seed, rnd, j, P[sm, ij, :])
            rows = (rows * P[:, ij, :][:, y].T).astype(np.float32)
            rows, e = rescale(rows)
            E = (E + e).astype(np.int32)
        qt = np.cumsum(rows.astype(np.float64), axis=1)[:, -1] / np.float64(S)       # ascending s
        with np.errstate(divide="ignore"):
            w = np.where(qt > 0, 1.0 / (np.float64(M) * qt), 0.0)
    return State(rows, E, w, E.astype(np.float64) * LN2, np.float64(st.base + cond[i]))


def terms(st, P):
    """fp64 [M, N]: - sum_y pt (log pt + o[m]) with pt = (1/S) Phat . P, 0 log 0 = 0 -- before the weights."""
    S, N, C = P.shape
    pt = (st.phat.astype(np.float64) @ P.astype(np.float64).reshape(S, N * C)) / S
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(pt > 0, pt * (np.log(pt) + st.o[:, None]), 0.0)
    return -t.reshape(st.M, N, C).sum(axis=2)


def joint(st, P):
    """fp64 [N]: H[i] = sum_m w[m] terms[m, i]."""
    return (st.w[:, None] * terms(st, P)).sum(axis=0)


def scores(st, P, cond):
    return joint(st, P) - cond - st.base


def entropies(P):
    """(cond, marg) fp64 [N] of fp32 P [S, N, C]."""
    p = P.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = -np.where(p > 0, p * np.log(p), 0.0).sum(axis=2).mean(axis=0)
        pb = p.mean(axis=0)
        marg = -np.where(pb > 0, pb * np.log(pb), 0.0).sum(axis=1)
    return cond, marg


def brute_joint_entropy(P, chosen, i):
    """The definition: H(y_chosen, y_i) = - sum over every label tuple of p log p, p = (1/S) sum_s prod P[s, row, label]."""
    S, N, C = P.shape
    p64 = P.astype(np.float64)
    rows = list(chosen) + [i]
    h = 0.0
    for ys in itertools.product(range(C), repeat=len(rows)):
        p = np.mean(np.prod([p64[:, r, y] for r, y in zip(rows, ys)], axis=0))
        if p > 0:
            h -= p * np.log(p)
    return h


def bound(S, H):
    """|H_dev - H_ref| <= (S + 4) 2^-23 (1 + |H_ref|): see tests/test_gpu_batchbald.py."""
    return (S + 4) * 2.0 ** -23 * (1.0 + np.abs(H))
