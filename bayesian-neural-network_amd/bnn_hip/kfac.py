"""F20: a Kronecker-factored (KFAC) Laplace posterior for MLP / MLP_Dropout (csrc/kfac.hip; include/bnn_hip.h F20) -- the
structured sibling of laplace.DiagLaplace.  Per layer, with Wbar = [W | b] [out, in + 1] and abar = [a ; 1]:

    A = sum_n a_n a_n^T,  s = sum_n a_n,  G = sum_r gz_r gz_r^T,  Abar = [[A, s], [s^T, N]],  H ~= (Abar (x) G) / N

(Martens & Grosse's expectation approximation; exact for N = 1), summed over every accumulated minibatch.  Once per fit
`decompose()` takes Abar / N = Q_A diag(lA) Q_A^T and G = Q_G diag(lG) Q_G^T in fp64.  In that eigenbasis the posterior is a
diagonal Gaussian with precisions lG_j lA_i + tau, so the evidence, the linearised (GLM) predictive and the weight draw reuse
the diagonal machinery on rotated operands.

One minibatch is DiagLaplace's chain with bnn_kfac_layer in bnn_laplace_layer's place: bnn_dense_fwd per layer ->
bnn_laplace_seed -> bnn_kfac_layer per layer top down (three layers: 7 launches, no parallel branches).  The GLM predictive
runs bnn_kfac_glm_rotate + bnn_kfac_glm_var per layer and then the unchanged bnn_laplace_glm_finish / _sample;
`sample_bank` fills a sgmcmc.WeightBank with matrix-normal draws (bnn_kfac_sample, two launches per layer and chunk) for the
bank's ensemble tools.

There is no `network()`: the posterior is correlated inside a layer, not mean-field, so it is no (mu, rho) of a
BayesianNetwork.  `sample_bank` is the route to the tools that consume weight draws."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .capture import word32
from .laplace import LaplaceBase
from .ops import BnnHipError
from .runtime import state, take_samples


class KronLaplace(LaplaceBase):
    """`la = mlp.laplace(structure="kron"); la.fit(loader); la.fit_prior_precision(); la.glm_predictive(x)`.  The accumulated
    tensors of layer l: A[l] [in, in], s[l] [in], G[l] [out, out] (float32, bit-symmetric); after decompose() Q_A[l]
    [in + 1, in + 1], Q_G[l] [out, out] (float32, eigenvectors in columns) and lam_A[l], lam_G[l] (float64; lam_A32 / lam_G32
    the same rounded to float32), eigenvalues clamped at 0.  Not mean-field: there is no network(); draw weights with
    sample_bank()."""

    def _allocate(self):
        dev, f32, f64 = self.device, torch.float32, torch.float64
        dims = [(d.linear.in_features, d.linear.out_features) for d in self.layers]
        self.A = [torch.zeros((i, i), dtype=f32, device=dev) for i, _ in dims]
        self.s = [torch.zeros(i, dtype=f32, device=dev) for i, _ in dims]
        self.G = [torch.zeros((o, o), dtype=f32, device=dev) for _, o in dims]
        # the decomposition lives in fixed buffers: a captured predictive keeps reading them after a refit
        self.Q_A = [torch.zeros((i + 1, i + 1), dtype=f32, device=dev) for i, _ in dims]
        self.Q_G = [torch.zeros((o, o), dtype=f32, device=dev) for _, o in dims]
        self.lam_A = [torch.zeros(i + 1, dtype=f64, device=dev) for i, _ in dims]
        self.lam_G = [torch.zeros(o, dtype=f64, device=dev) for _, o in dims]
        self.lam_A32 = [torch.zeros(i + 1, dtype=f32, device=dev) for i, _ in dims]
        self.lam_G32 = [torch.zeros(o, dtype=f32, device=dev) for _, o in dims]
        self._decomposed = False

    def _accumulated(self):
        return self.A + self.s + self.G + [self.record]

    def _invalidate(self):
        self._decomposed = False

    def _curvature_launch(self, i, x, gy, *, g_x, y, gx_mask, math_mode):
        ops.kfac_layer(x, gy, self.layers[i].linear.weight.detach(), a=self.A[i], s=self.s[i], g=self.G[i], g_x=g_x, y=y,
                       gx_mask=gx_mask, math_mode=math_mode)

    # ---- the eigenbasis
    @staticmethod
    def _eigh(m: torch.Tensor):
        """fp64 eigh on the device; on the host where this build's device solver raises (once per fit)."""
        try:
            return torch.linalg.eigh(m)
        except RuntimeError:
            lam, q = torch.linalg.eigh(m.cpu())
            return lam.to(m.device), q.to(m.device)

    def decompose(self):
        """Abar / N and G of every layer -> (Q, lambda), eigenvalues below 0 set to 0.  Called lazily by whatever needs the
        eigenbasis; accumulate / reset invalidate it.  Returns self."""
        if self._decomposed:
            return self
        N = self.n_rows
        if N < 1:
            raise BnnHipError("KronLaplace: nothing accumulated yet; call fit() or accumulate() first")
        with torch.no_grad():
            for l, (A, s, G) in enumerate(zip(self.A, self.s, self.G)):
                n = A.shape[0]
                abar = torch.empty((n + 1, n + 1), dtype=torch.float64, device=self.device)
                abar[:n, :n] = A
                abar[:n, n] = s
                abar[n, :n] = s
                abar[n, n] = float(N)
                abar /= float(N)
                for m, Q, lam, lam32 in ((abar, self.Q_A[l], self.lam_A[l], self.lam_A32[l]),
                                         (G.double(), self.Q_G[l], self.lam_G[l], self.lam_G32[l])):
                    ev, q = self._eigh(m)
                    lam.copy_(ev.clamp_min(0.0))
                    lam32.copy_(lam)
                    Q.copy_(q)
        self._decomposed = True
        return self

    # ---- the prior precision
    def _evidence(self, precisions, best_index, best):
        self.decompose()
        taus = [float(t) for t in np.asarray(precisions, dtype=np.float64).reshape(-1)]
        return ops.kfac_evidence(self.params[0::2], self.params[1::2], self.lam_A, self.lam_G, taus, record=self.record,
                                 best_index=best_index, best=best)

    # ---- the linearised (GLM) predictive: LaplaceBase's interface over this structure's two launches per layer
    def _glm_buffers(self, chain):
        f32 = dict(dtype=torch.float32, device=self.device)
        chain.at = [torch.empty((chain.B, d.linear.in_features + 1), **f32) for d in self.layers]
        chain.gt = [torch.empty((chain.R, d.linear.out_features), **f32) for d in self.layers]

    def _glm_launch(self, chain, i, x, gy, *, g_x, y, gx_mask, precision, precision_device, math_mode):
        ops.kfac_glm_rotate(x, gy, self.layers[i].linear.weight.detach(), q_a=self.Q_A[i], q_g=self.Q_G[i], at=chain.at[i],
                            gt=chain.gt[i], g_x=g_x, y=y, gx_mask=gx_mask, math_mode=math_mode)
        ops.kfac_glm_var(chain.at[i], chain.gt[i], self.lam_A[i], self.lam_G[i], cov_part=chain.parts[i], precision=precision,
                         precision_device=precision_device)

    def _glm_ready(self):
        """The eigenbasis of what has been accumulated, before every GLM call and every replay of a captured predictive (never
        inside a capture: eigh is host-driven).  The captured launches read the decomposition's fixed buffers, so a replay
        after a refit sees the new posterior; decompose() returns at once while the basis is current."""
        self.decompose()

    # ---- weight draws
    def members_per_launch(self, members: int, budget_bytes: int = 1 << 28) -> int:
        """Draws per bnn_kfac_sample call: as many as `budget_bytes` of the widest layer's T [members, out, in + 1] workspace
        allow (at least 1, at most `members`) -- WeightBank.rows_per_launch's rule for the launch's one large buffer."""
        per_member = 4 * max(d.linear.out_features * (d.linear.in_features + 1) for d in self.layers)
        return int(max(1, min(int(members), int(budget_bytes) // per_member)))

    def sample_bank(self, members: int, bank=None, sample_offset: Optional[int] = None, *, prior_precision: Optional[float] = None,
                    budget_bytes: int = 1 << 28):
        """Fill slots 0 .. members - 1 of a sgmcmc.WeightBank (a new one of that capacity by default) with draws
        Wbar_s = Wbar + Q_G (E_s o Sigma) Q_A^T, Sigma_ji = (lG_j lA_i + tau)^-1/2, and return the bank:
        bank.predict_mc / predictive / score / evaluate / predictive_graph then run unchanged.  Draw s uses the global sample
        index sample_offset + s (by default the next `members` of the process-wide counter), whatever the chunking: the same
        offset gives the same bits.  tau defaults to the word fit_prior_precision chose.  A bank passed in has its slots
        0 .. members - 1 overwritten; its `collected` word is raised to `members` if it held fewer and is otherwise left alone,
        so a sampler that files into the same ring keeps its next slot -- and will overwrite draws in turn: give the draws a
        bank of their own unless that mixture is wanted."""
        from .sgmcmc import WeightBank, _set_word
        M = int(members)
        if M < 1:
            raise BnnHipError(f"KronLaplace.sample_bank: members must be >= 1, got {members}")
        self._check_math()
        if bank is None:
            bank = WeightBank(self.mlp, M)
        elif bank.capacity < M or bank.shapes != [tuple(p.shape) for p in self.params]:
            raise BnnHipError(f"KronLaplace.sample_bank: the bank must hold {M} members of this network's parameter shapes")
        self.decompose()
        tau, tau_dev = self._tau(prior_precision, "sample_bank")
        base = take_samples(M) if sample_offset is None else int(sample_offset)
        chunk = self.members_per_launch(M, budget_bytes)
        ws = None
        with torch.no_grad():
            for first in range(0, M, chunk):
                m = min(chunk, M - first)
                for l, d in enumerate(self.layers):
                    ws = ops.kfac_sample(d.linear.weight.detach(), d.linear.bias.detach(), self.Q_A[l], self.Q_G[l], self.lam_A[l],
                                         self.lam_G[l], bank.buffer, bank._w_off[l], bank._b_off[l], members=m, first=first, layer=l,
                                         seed=state.seed, sample_base=word32(base + first) & 0xFFFFFFFF, precision=tau,
                                         precision_device=tau_dev, workspace=ws)
        if bank.count() < M:                                                  # (a fuller bank, or a wrapped ring, keeps its word)
            _set_word(bank.collected, M)
        return bank
