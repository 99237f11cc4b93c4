"""TEST INFRASTRUCTURE: numpy restatement of the IVON entries (include/bnn_hip.h F24; csrc/ivon.hip) -- the noise stream from the
oracle's Philox and Box-Muller on counter word 3 = 6, the draw, the fold and the step in fp32 with their fused multiply-adds
formed exactly and in the kernel's chain order, the fp64 running product beta1^t with its one fused use, a chain that walks the
steps t and the samples s, and a direct fp64 transcription of the published algorithm (Shen et al. 2024, Algorithm 1).  Nothing
here imports the product; tests compare the product against it."""
from fractions import Fraction

import numpy as np

from oracle import bnn_oracle as O
from sgmcmc_ref import fma32, layout  # noqa: F401  (the exact fp32 fma and the bank's layout, restated there)

MAX_TENSORS = 16
MAX_SAMPLES = 8
MAX_MEMBERS = 64
WORD3 = 6                      # counter word 3 of the IVON noise stream
F32 = np.float32
M32 = 0xFFFFFFFF


def noise(seed, q, tensor, numel):
    """float32[numel]: element i of tensor `tensor` of draw q from counter (i >> 2, q, tensor, 6), slot i & 3."""
    g = np.arange((int(numel) + 3) // 4, dtype=np.uint64).astype(np.uint32)
    r0, r1, r2, r3 = O.philox4x32(g, np.uint32(int(q) & M32), np.uint32(tensor), np.uint32(WORD3), seed & M32, (seed >> 32) & M32)
    n0, n1 = O.box_muller(r0, r1)
    n2, n3 = O.box_muller(r2, r3)
    return np.ascontiguousarray(np.stack([n0, n1, n2, n3], axis=-1).reshape(-1)[:numel])


def draw_index(step, samples, s):
    """q = t * S + s in the 32-bit word the kernels compute it in."""
    return ((int(step) & M32) * int(samples) + int(s)) & M32


def lr_eff(lr, hess_init, weight_decay, rescale_lr=True):
    return lr * (hess_init + weight_decay) if rescale_lr else lr


def default_loss_scale(loss, batch, sigma=None):
    if loss == "mse" and sigma is not None:
        return 1.0 / (2.0 * sigma ** 2 * batch)
    return 1.0 / batch


def fma64(a, b, c):
    """fp64 fma(a, b, c) of Python floats, correctly rounded (exact rational arithmetic, one rounding)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def inv_bias_correction(prod, beta1):
    """ib = (float)(1 / fma(-P, beta1, 1)) with P = beta1^t the running product BEFORE the step: 1 / (1 - beta1^(t+1))."""
    return F32(1.0 / fma64(-float(prod), float(beta1), 1.0))


def scale(h, ess, delta):
    """(hd, r, sigma) in float32: hd = h + delta, r = sqrt(ess * hd), sigma = 1 / r."""
    hd = (np.asarray(h, dtype=F32) + F32(delta)).astype(F32)
    r = np.sqrt((F32(ess) * hd).astype(F32)).astype(F32)
    return hd, r, (F32(1.0) / r).astype(F32)


def draw(m, h, eps, ess, delta):
    """theta = fma(sigma, eps, m)."""
    return fma32(scale(h, ess, delta)[2], np.asarray(eps, dtype=F32), np.asarray(m, dtype=F32))


def fold(g, eps_prev, h, acc_g, acc_h, ess, delta, first):
    """(acc_g', acc_h') after folding the previous sample's gradient g drawn with eps_prev; `first`: sample 1 (no read)."""
    g = np.asarray(g, dtype=F32)
    er = (np.asarray(eps_prev, dtype=F32) * scale(h, ess, delta)[1]).astype(F32)
    if first:
        return g.copy(), (g * er).astype(F32)
    return (np.asarray(acc_g, dtype=F32) + g).astype(F32), fma32(g, er, acc_h)


def constants(*, ess, weight_decay, beta1, beta2, loss_scale, samples, clip_radius=np.inf):
    """The launch's fp32 constants, formed in fp64 in the host's order and rounded once."""
    S, rho = float(samples), 1.0 - float(beta2)
    return dict(ess=F32(ess), delta=F32(weight_decay), beta1=F32(beta1), c1=F32((1.0 - float(beta1)) * float(loss_scale) / S),
                cS=F32(float(loss_scale) / S), rho=F32(rho), c2=F32(0.5 * rho * rho), clip=F32(clip_radius))


def step(m, g, h, gm, eps, acc_g, acc_h, k, ib, lr, multi, clip):
    """(p', h', gm') in float32 in the kernel's chain order; k = constants(...), ib = inv_bias_correction(...), lr the rate used."""
    m, g, h, gm, eps = (np.asarray(t, dtype=F32) for t in (m, g, h, gm, eps))
    hd, r, _ = scale(h, k["ess"], k["delta"])
    er = (eps * r).astype(F32)
    gs = (np.asarray(acc_g, dtype=F32) + g).astype(F32) if multi else g
    hs = fma32(g, er, acc_h) if multi else (g * er).astype(F32)
    gm2 = fma32(k["beta1"], gm, (k["c1"] * gs).astype(F32))
    d = fma32(-k["cS"], hs, h)
    h2 = fma32(k["c2"], ((d * d).astype(F32) / hd).astype(F32), fma32(-k["rho"], d, h))
    u = (fma32(k["delta"], m, (gm2 * F32(ib)).astype(F32)) / (h2 + k["delta"]).astype(F32)).astype(F32)
    if clip:
        u = np.minimum(np.maximum(u, -k["clip"]), k["clip"]).astype(F32)
    return fma32(-F32(lr), u, m), h2, gm2


class Chain:
    """The optimiser on lists of float32 arrays: step t runs draw(0, eps) .. draw(S - 1, eps, grads of the previous sample), then
    step(grads of the last sample).  The state (mean, hess, gm, acc_g, acc_h) as flat arrays in the bank's layout, the padding
    filled with `pad` and never written.  `lr` is the rate used (lr_eff)."""

    def __init__(self, params, *, lr, ess, hess_init=1.0, beta1=0.9, beta2=0.99999, weight_decay=1e-4, samples=1,
                 clip_radius=np.inf, loss_scale=1.0, step=0, prod=1.0, pad=0.0):
        self.p = [np.array(t, dtype=F32) for t in params]
        self.lr, self.S, self.t, self.prod, self.beta1 = lr, int(samples), int(step) & M32, float(prod), float(beta1)
        self.k = constants(ess=ess, weight_decay=weight_decay, beta1=beta1, beta2=beta2, loss_scale=loss_scale, samples=samples,
                           clip_radius=clip_radius)
        self.clip = bool(np.isfinite(clip_radius))
        self.offs, self.stride = layout([t.size for t in self.p])
        self.sl = [slice(o, o + t.size) for o, t in zip(self.offs, self.p)]
        self.mean, self.hess, self.gm = (np.full(self.stride, pad, F32) for _ in range(3))
        self.acc_g, self.acc_h = (np.full(self.stride, pad, F32), np.full(self.stride, pad, F32)) if self.S > 1 else (None, None)
        for sl in self.sl:
            self.mean[sl], self.hess[sl], self.gm[sl] = 0, hess_init, 0
            if self.S > 1:
                self.acc_g[sl], self.acc_h[sl] = 0, 0
        self.s, self.eps = 0, None

    def q(self, s=None):
        return draw_index(self.t, self.S, self.s if s is None else s)

    def draw(self, s, eps, grads=None):
        """Sample s: `eps` a list of noise arrays (one per tensor) of draw q(s); `grads`: sample s - 1's (s >= 1)."""
        assert s == self.s < self.S
        for t, sl in enumerate(self.sl):
            if s == 0:
                self.mean[sl] = self.p[t].reshape(-1)
            else:
                self.acc_g[sl], self.acc_h[sl] = fold(np.reshape(grads[t], -1), np.reshape(self.eps[t], -1), self.hess[sl],
                                                      self.acc_g[sl], self.acc_h[sl], self.k["ess"], self.k["delta"], s == 1)
            self.p[t] = draw(self.mean[sl], self.hess[sl], np.reshape(eps[t], -1), self.k["ess"],
                             self.k["delta"]).reshape(self.p[t].shape)
        self.eps, self.s = [np.asarray(e, dtype=F32) for e in eps], s + 1

    def step(self, grads):
        assert self.s == self.S
        ib = inv_bias_correction(self.prod, self.beta1)
        for t, sl in enumerate(self.sl):
            p, h, gm = step(self.mean[sl], np.reshape(grads[t], -1), self.hess[sl], self.gm[sl], np.reshape(self.eps[t], -1),
                            None if self.S == 1 else self.acc_g[sl], None if self.S == 1 else self.acc_h[sl], self.k, ib, self.lr,
                            self.S > 1, self.clip)
            self.p[t], self.hess[sl], self.gm[sl] = p.reshape(self.p[t].shape), h, gm
        self.prod *= self.beta1
        self.t = (self.t + 1) & M32
        self.s = 0

    def sigma(self, t):
        return scale(self.hess[self.sl[t]], self.k["ess"], self.k["delta"])[2]


class Published:
    """Shen et al. 2024, Algorithm 1, transcribed directly in fp64 for one flat array: theta - m is formed, the bias correction
    is a power, the sample means are sums divided by S, nothing is reordered for the kernel's sake.

        ghat = mean_s g_s;   hhat = mean_s g_s (theta_s - m) / sigma^2;   gm = b1 gm + (1 - b1) ghat
        h' = b2 h + (1 - b2) hhat + (1 - b2)^2 (h - hhat)^2 / (2 (h + delta))
        m = m - lr clip((gm / (1 - b1^t) + delta m) / (h' + delta));   sigma = 1 / sqrt(ess (h' + delta))      t counted from 1"""

    def __init__(self, m, *, lr, ess, hess_init=1.0, beta1=0.9, beta2=0.99999, weight_decay=1e-4, clip_radius=np.inf,
                 loss_scale=1.0):
        self.m = np.array(m, dtype=np.float64)
        self.h = np.full_like(self.m, hess_init)
        self.gm = np.zeros_like(self.m)
        self.lr, self.ess, self.b1, self.b2, self.delta, self.clip, self.c = lr, ess, beta1, beta2, weight_decay, clip_radius, loss_scale
        self.t = 0

    def sigma(self):
        return 1.0 / np.sqrt(self.ess * (self.h + self.delta))

    def theta(self, eps):
        return self.m + self.sigma() * np.asarray(eps, dtype=np.float64)

    def step(self, thetas, grads):
        """`thetas`, `grads`: the S draws and the gradients of the SUM loss there (scaled here by loss_scale)."""
        S = len(grads)
        sig2 = self.sigma() ** 2
        ghat = sum(self.c * np.asarray(g, dtype=np.float64) for g in grads) / S
        hhat = sum(self.c * np.asarray(g, dtype=np.float64) * (th - self.m) / sig2 for g, th in zip(grads, thetas)) / S
        self.t += 1
        self.gm = self.b1 * self.gm + (1.0 - self.b1) * ghat
        hd = self.h + self.delta
        self.hhat = hhat
        self.h = self.b2 * self.h + (1.0 - self.b2) * hhat + 0.5 * (1.0 - self.b2) ** 2 * (self.h - hhat) ** 2 / hd
        u = (self.gm / (1.0 - self.b1 ** self.t) + self.delta * self.m) / (self.h + self.delta)
        self.u = np.clip(u, -self.clip, self.clip)
        self.m = self.m - self.lr * self.u
