"""TEST INFRASTRUCTURE: numpy restatement of the SG-MCMC entries (include/bnn_hip.h F19; csrc/sgmcmc.hip) -- the noise stream from
the oracle's Philox and Box-Muller, the fp32 update rule with its fused multiply-adds formed exactly, a chain that steps a
schedule table and files its samples into the ring, the bank's layout, and the stationary covariance of the rule on a Gaussian
target.  Nothing here imports the product; tests compare the product against it."""
import numpy as np

from oracle import bnn_oracle as O

MAX_TENSORS = 16
WORD3 = 3                      # counter word 3 of the SG-MCMC noise stream
F32 = np.float32


def noise(seed, tensor, step, numel):
    """float32[numel]: element i from counter (i >> 2, step, tensor, 3), key (seed_lo, seed_hi), slot i & 3."""
    groups = (int(numel) + 3) // 4
    g = np.arange(groups, dtype=np.uint64).astype(np.uint32)
    r0, r1, r2, r3 = O.philox4x32(g, np.uint32(int(step) & 0xFFFFFFFF), np.uint32(tensor), np.uint32(WORD3),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    n0, n1 = O.box_muller(r0, r1)
    n2, n3 = O.box_muller(r2, r3)
    return np.ascontiguousarray(np.stack([n0, n1, n2, n3], axis=-1).reshape(-1)[:numel])


def fma32(a, b, c):
    """fp32 fma(a, b, c) of float32 arrays, correctly rounded: the product is exact in fp64; the fp64 sum is rounded to odd
    (TwoSum gives its exact error), after which the rounding to fp32 is the only one that counts."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    need = (e != 0) & even
    s = np.where(need, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def update(p, v, grad, eps, grad_scale, tau, a, b, c):
    """(p', v') in float32: g = fma(grad_scale, grad, tau p); v' = fma(c, eps, fma(-a, g, b v)); p' = p + v'."""
    p, v, grad, eps = (np.asarray(t, dtype=F32) for t in (p, v, grad, eps))
    gs, tau, a, b, c = (F32(t) for t in (grad_scale, tau, a, b, c))
    g = fma32(gs, grad, tau * p)
    v2 = fma32(c, eps, fma32(-a, g, b * v))
    return (p + v2).astype(F32), v2


def learning_rates(lr, thin=1, cycle_length=None):
    if cycle_length is None:
        return np.full(thin, float(lr))
    j = np.arange(cycle_length, dtype=np.float64)
    return float(lr) / 2.0 * (np.cos(np.pi * j / cycle_length) + 1.0)


def table(lrs, temperature=1.0, friction=None, flags=None):
    """float32 [L, 4] (a, b, c, flag) from fp64 step sizes, rounded once."""
    lrs = np.asarray(lrs, dtype=np.float64)
    t = np.zeros((len(lrs), 4), dtype=np.float64)
    if friction is None:
        t[:, 0], t[:, 2] = lrs / 2.0, np.sqrt(lrs * temperature)
    else:
        t[:, 0], t[:, 1], t[:, 2] = lrs, 1.0 - friction, np.sqrt(2.0 * friction * lrs * temperature)
    if flags is not None:
        t[:, 3] = np.asarray(flags, dtype=np.float64)
    return t.astype(F32)


def cycle_flags(cycle_length, thin, collect_fraction):
    """Rows of a cycle that collect: the last max(1, floor(fraction L)) rows, every thin-th counted back from the last."""
    n = max(1, int(np.floor(collect_fraction * cycle_length + 1e-9)))
    return np.array([j >= cycle_length - n and (cycle_length - 1 - j) % thin == 0 for j in range(cycle_length)])


def layout(numels):
    """(offsets, stride): every tensor of a member starts at a multiple of 64 elements."""
    offs, tot = [], 0
    for n in numels:
        offs.append(tot)
        tot += (n + 63) // 64 * 64
    return offs, tot


def ring_slot(collected, capacity):
    return (collected & 0xFFFFFFFF) % capacity


class Chain:
    """The sampler on lists of float32 arrays: step word, table row k % L, the ring."""

    def __init__(self, params, tab, *, grad_scale, tau, momentum, burn_in=0, bank=None, seed=0, step=0, collected=0):
        self.p = [np.array(t, dtype=F32) for t in params]
        self.v = [np.zeros_like(t) for t in self.p] if momentum else None
        self.tab, self.gs, self.tau, self.burn_in, self.seed = np.asarray(tab, dtype=F32), grad_scale, tau, burn_in, seed
        self.bank, self.k, self.collected = bank, step, collected
        self.offs, self.stride = layout([t.size for t in self.p])
        self.rows_used = []

    def step(self, grads, eps=None):
        """eps: a list of arrays, None for the Philox stream at the step word, or "zero"."""
        k = self.k & 0xFFFFFFFF
        j = k % len(self.tab)
        a, b, c, flag = self.tab[j]
        self.rows_used.append(j)
        for t, p in enumerate(self.p):
            if eps is None:
                e = noise(self.seed, t, k, p.size).reshape(p.shape)
            else:
                e = np.zeros_like(p) if isinstance(eps, str) else eps[t]
            v = np.zeros_like(p) if self.v is None else self.v[t]
            p2, v2 = update(p, v, grads[t], e, self.gs, self.tau, a, b, c)
            self.p[t] = p2
            if self.v is not None:
                self.v[t] = v2
        if self.bank is not None and k >= self.burn_in and flag != 0:
            m = ring_slot(self.collected, self.bank.shape[0])
            for o, p in zip(self.offs, self.p):
                self.bank[m, o:o + p.size] = p.reshape(-1)
            self.collected += 1
        self.k += 1


def stationary(a, b, c, tau, iters=100000, tol=1e-15):
    """(Sigma, A) of the linear chain (p, v)' = A (p, v) + c eps (1, 1) at grad = 0: Sigma = A Sigma A^T + c^2 11^T iterated to
    convergence in fp64.  A = [[1 - a tau, b], [-a tau, b]]."""
    a, b, c, tau = (float(t) for t in (a, b, c, tau))
    A = np.array([[1.0 - a * tau, b], [-a * tau, b]])
    Q = c * c * np.ones((2, 2))
    S = Q.copy()
    for _ in range(iters):
        S2 = A @ S @ A.T + Q
        if np.abs(S2 - S).max() <= tol * np.abs(S2).max():
            return S2, A
        S = S2
    raise RuntimeError("the chain's covariance did not converge")


def chain_statistics(run, n=16384, steps=200):
    """run(k) -> the float32 state p after step k (k = 0 .. steps - 1), from zero.  Returns (var of the last state, its mean,
    the lag-1 correlation of the last two states) in fp64."""
    prev = last = None
    for k in range(steps):
        prev, last = last, np.asarray(run(k), dtype=np.float64).copy()
    assert last.size == n
    var = last.var()
    lag1 = ((last - last.mean()) * (prev - prev.mean())).mean() / np.sqrt(var * prev.var())
    return var, last.mean(), lag1


def check_statistics(var, mean, lag1, tab_row, tau, n=16384):
    """The three bounds of the issue against the stationary law of the rounded table row."""
    a, b, c = (float(t) for t in tab_row[:3])
    S, A = stationary(a, b, c, tau)
    rho = max(abs(np.linalg.eigvals(A)))
    assert rho ** 200 < 1e-15
    assert abs(var / S[0, 0] - 1.0) < 0.05, (var, S[0, 0])
    assert abs(mean) < 4.0 * np.sqrt(S[0, 0] / n), (mean, S[0, 0])
    want = (A @ S)[0, 0] / S[0, 0]
    assert abs(lag1 - want) < 0.01, (lag1, want)
    return var / S[0, 0], lag1, want
