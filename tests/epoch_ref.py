"""TEST INFRASTRUCTURE: CPU restatements of the device epoch loader (include/bnn_hip.h F8) -- the epoch permutation and
the staging of one minibatch -- in numpy, with the oracle's Philox restatement for the keys."""
import numpy as np

from oracle import bnn_oracle as O

COUNTER_WORDS = (2, 1)          # words 2 and 3 of the permutation stream's counter (p >> 2, epoch, 2, 1)


def keys(seed, epoch, N):
    """uint32 [N]: key_p = word (p & 3) of Philox4x32-R((p >> 2, epoch, 2, 1), seed)."""
    p = np.arange(N, dtype=np.uint32)
    r = np.stack(O.philox4x32(p >> 2, np.uint32(epoch), COUNTER_WORDS[0], COUNTER_WORDS[1], seed & 0xFFFFFFFF,
                              (seed >> 32) & 0xFFFFFFFF), axis=-1)
    return r[np.arange(N), p & 3].astype(np.uint32)


def permutation(seed, epoch, N):
    """int32 [N]: the positions sorted by (key_p, p)."""
    k = keys(seed, epoch, N).astype(np.uint64)
    pairs = (k << np.uint64(32)) | np.arange(N, dtype=np.uint64)
    return np.argsort(pairs, kind="stable").astype(np.int32)


def bf16_bits(v):
    """uint16 bits of the round-to-nearest-even bf16 of fp32 `v` (finite inputs)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def beta(M, j):
    """The reference's expression (class_task.py:70), then one rounding to fp32."""
    return np.float32(2 ** (M - (j + 1)) / (2 ** M - 1))


def stage(x, y, j, B, order=None, M=None):
    """(x_out fp32 [B, d], x16 bits uint16 [B, d], y_out [B] / [B, k], beta_j or None) of minibatch j: x [N, d] fp32 or
    uint8 (u / 255 in fp32: ToTensor), order None = identity."""
    idx = np.arange(j * B, (j + 1) * B) if order is None else np.asarray(order)[j * B:(j + 1) * B]
    rows = x[idx]
    xo = (rows.astype(np.float32) / np.float32(255.0)) if x.dtype == np.uint8 else rows.astype(np.float32)
    return xo, bf16_bits(xo), y[idx], (beta(M, j) if M is not None else None)
