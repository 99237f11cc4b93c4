"""TEST INFRASTRUCTURE: numpy restatement of the SWAG entries (include/bnn_hip.h F22; csrc/swag.hip) -- the two noise streams from
the oracle's Philox and Box-Muller, the SGD step and Welford's moment update in fp32 with their fused multiply-adds formed
exactly, a chain that walks start / every and the ring of deviations, the draw in fp32 in the kernel's chain order, and the exact
covariance of the draw in fp64.  Nothing here imports the product; tests compare the product against it."""
import numpy as np

from oracle import bnn_oracle as O
from sgmcmc_ref import fma32, layout  # noqa: F401  (the exact fma and the bank's layout, restated there)

MAX_TENSORS = 16
MAX_RANK = 32
MAX_MEMBERS = 64
WORD3 = 5                      # counter word 3 of both SWAG noise streams
Z2_STREAM = MAX_TENSORS        # counter word 2 of z2 (the tensors use 0 .. MAX_TENSORS - 1)
F32 = np.float32


def _normals(groups, q, stream, seed):
    g = np.arange(groups, dtype=np.uint64).astype(np.uint32)
    r0, r1, r2, r3 = O.philox4x32(g, np.uint32(int(q) & 0xFFFFFFFF), np.uint32(stream), np.uint32(WORD3), seed & 0xFFFFFFFF,
                                   (seed >> 32) & 0xFFFFFFFF)
    n0, n1 = O.box_muller(r0, r1)
    n2, n3 = O.box_muller(r2, r3)
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(-1)


def z1(seed, q, tensor, numel):
    """float32[numel]: element i of tensor `tensor` of draw q from counter (i >> 2, q, tensor, 5), slot i & 3."""
    return np.ascontiguousarray(_normals((int(numel) + 3) // 4, q, tensor, seed)[:numel])


def z2(seed, q, rank):
    """float32[rank]: z2[q][j] from counter (j >> 2, q, MAX_TENSORS, 5), slot j & 3."""
    return np.ascontiguousarray(_normals((int(rank) + 3) // 4, q, Z2_STREAM, seed)[:rank])


def sgd_update(p, v, g, lr, mu=0.0, wd=0.0):
    """(p', v') in float32: g' = wd != 0 ? fma(wd, p, g) : g; u = v is None ? g' : (v' = fma(mu, v, g')); p' = fma(-lr, u, p)."""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    gg = fma32(F32(wd), p, g) if F32(wd) != 0 else g
    v2 = None if v is None else fma32(F32(mu), np.asarray(v, dtype=F32), gg)
    return fma32(-F32(lr), gg if v is None else v2, p), v2


def collects(k, start, every):
    k &= 0xFFFFFFFF
    return k >= start and (k - start + 1) % every == 0


def welford(p, mean, m2, n):
    """(mean', m2', deviation) in float32 with r = 1 / (float)(n + 1) correctly rounded."""
    p, mean, m2 = (np.asarray(t, dtype=F32) for t in (p, mean, m2))
    r = F32(1.0) / F32(n + 1)
    d = (p - mean).astype(F32)
    mean2 = fma32(d, r, mean)
    dv = (p - mean2).astype(F32)
    return mean2, fma32(d, dv, m2), dv


class Chain:
    """The collector on lists of float32 arrays; the moments as flat arrays in the bank's layout (given, or zeros)."""

    def __init__(self, params, *, lr, mu=0.0, wd=0.0, momentum=False, start=0, every=1, rank=0, step=0, count=0, mean=None, m2=None,
                 dev=None):
        self.p = [np.array(t, dtype=F32) for t in params]
        self.v = [np.zeros_like(t) for t in self.p] if momentum else None
        self.lr, self.mu, self.wd, self.start, self.every, self.K = lr, mu, wd, start, every, rank
        self.k, self.n = step, count
        self.offs, self.stride = layout([t.size for t in self.p])
        self.mean = np.zeros(self.stride, F32) if mean is None else mean
        self.m2 = np.zeros(self.stride, F32) if m2 is None else m2
        self.dev = (np.zeros((rank, self.stride), F32) if dev is None else dev) if rank else None
        self.collected_at = []

    def step(self, grads):
        col = collects(self.k, self.start, self.every)
        for t, p in enumerate(self.p):
            p2, v2 = sgd_update(p, None if self.v is None else self.v[t], grads[t], self.lr, self.mu, self.wd)
            self.p[t] = p2
            if self.v is not None:
                self.v[t] = v2
            if col:
                sl = slice(self.offs[t], self.offs[t] + p.size)
                a, s, dv = welford(p2.reshape(-1), self.mean[sl], self.m2[sl], self.n)
                self.mean[sl], self.m2[sl] = a, s
                if self.K:
                    self.dev[self.n % self.K, sl] = dv
        if col:
            self.collected_at.append(self.k)
            self.n += 1
        self.k += 1

    def collect(self, iterate):
        """Fold a given iterate (a list of arrays) in, as a collecting step does after its update."""
        for t, p in enumerate(iterate):
            sl = slice(self.offs[t], self.offs[t] + p.size)
            a, s, dv = welford(np.asarray(p, dtype=F32).reshape(-1), self.mean[sl], self.m2[sl], self.n)
            self.mean[sl], self.m2[sl] = a, s
            if self.K:
                self.dev[self.n % self.K, sl] = dv
        self.n += 1


def coefficients(scale, low_rank=True):
    """(c_d, c_lr[0 .. MAX_RANK]) in float32 from fp64, rounded once."""
    c_lr = np.zeros(MAX_RANK + 1, dtype=np.float64)
    if low_rank:
        for e in range(2, MAX_RANK + 1):
            c_lr[e] = np.sqrt(scale / (2.0 * (e - 1)))
    return F32(np.sqrt(scale / 2.0 if low_rank else scale)), c_lr.astype(F32)


def draw(mean, m2, dev, n, z1v, z2v, *, scale=1.0, low_rank=True, var_clamp=1e-30):
    """One member over flat float32 arrays (any common shape; dev [K, ...], z2v [K]) in the kernel's order."""
    mean, m2, z1v = (np.asarray(t, dtype=F32) for t in (mean, m2, z1v))
    c_d, c_lr = coefficients(scale, low_rank)
    r = F32(1.0) / F32(n) if n else F32(0.0)
    s = np.sqrt(np.maximum((m2 * r).astype(F32), F32(var_clamp))).astype(F32)
    theta = fma32((c_d * s).astype(F32), z1v, mean)
    if low_rank:
        keff = min(n, dev.shape[0])
        acc = np.zeros_like(mean)
        for j in range(keff):
            acc = fma32(dev[j], F32(z2v[j]), acc)
        theta = fma32(c_lr[keff], acc, theta)
    return theta


def covariance(m2, dev, n, *, scale=1.0, low_rank=True, var_clamp=1e-30):
    """The draw's exact covariance in fp64 from the float32 statistics and the ROUNDED coefficients the kernel uses:
    c_d^2 diag(s^2) + c_lr[Keff]^2 D^T D, s the kernel's float32 sqrt(max(m2 / n, var_clamp))."""
    c_d, c_lr = coefficients(scale, low_rank)
    m2 = np.asarray(m2, dtype=F32)
    s = np.sqrt(np.maximum((m2 * (F32(1.0) / F32(n))).astype(F32), F32(var_clamp))).astype(F32)
    cs = (c_d * s).astype(F32).astype(np.float64)
    S = np.diag(cs * cs)
    if low_rank:
        keff = min(n, dev.shape[0])
        D = np.asarray(dev[:keff], dtype=np.float64)
        S = S + float(c_lr[keff]) ** 2 * (D.T @ D)
    return S


def swag_covariance(var, dev, keff, scale=1.0):
    """The paper's scale * (diag(var) / 2 + D^T D / (2 (Keff - 1))) in fp64."""
    D = np.asarray(dev[:keff], dtype=np.float64)
    return scale * (np.diag(np.asarray(var, dtype=np.float64)) / 2.0 + D.T @ D / (2.0 * (keff - 1)))
