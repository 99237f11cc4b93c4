"""F14: fine-tuning a posthoc.CompressedNetwork -- one Bayes-by-backprop step over the SURVIVING weights only, captured as
ONE hipGraph (prune, fine-tune, prune again).  The pattern stays fixed: a pruned weight or bias is exactly zero in every
sample, is in neither ELBO sum and receives no gradient.  The posterior, the epsilon map and the arithmetic of the forward
are the ones F13 defined (bnn_sparse_fwd); a network compressed from a local-reparameterisation net trains with the same
weight-space draw and the sampled log q - log p estimator.

The captured step: bnn_sparse_elbo_terms (log q, log p of the kept parameters), bnn_sparse_fwd x 3, bnn_elbo_finalize
(the NLL), bnn_elbo_loss_nll_bwd (loss, backward seeds, d nll / d logits), bnn_sparse_bwd x 3 (epsilon regenerated),
bnn_adam_step (which also advances the MC-sample counter), bnn_sparse_sigma_refresh.  It has train.GraphedTrainStep's
contract -- static x, y, beta; the optimiser's shared device sample counter; warm-up steps whose effects are undone;
step() / replay() returning the static (loss, mean log p, mean log q, nll); sync_lr honoured -- and the attributes
epoch.EpochRunner reads, so an EpochRunner drives it as it drives a GraphedTrainStep.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops
from .capture import SampleCounter, grad_bucket, snapshot, warm_up
from .optim import FusedAdam
from .runtime import state


def csc_view(row_ptr: torch.Tensor, col: torch.Tensor, nnz: int, in_features: int):
    """The CSC view of a CSR pattern, with torch ops on the tensors' device (built once per step object; not on the step's
    path): (col_ptr int32 [in + 1], row int16 holding uint16 bits [max(nnz, 1)], perm int32 [max(nnz, 1)]) -- the entries
    sorted by column, rows ascending within a column (a stable sort of col), perm the CSR position of each."""
    dev = row_ptr.device
    out = row_ptr.numel() - 1
    counts = (row_ptr[1:] - row_ptr[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(out, device=dev), counts, output_size=nnz)
    cols = col[:nnz].to(torch.int64) & 0xFFFF
    _, perm = torch.sort(cols, stable=True)
    col_ptr = torch.zeros(in_features + 1, dtype=torch.int64, device=dev)
    col_ptr[1:] = torch.cumsum(torch.bincount(cols, minlength=in_features), 0)
    row16 = torch.zeros(max(nnz, 1), dtype=torch.int16, device=dev)
    perm32 = torch.zeros(max(nnz, 1), dtype=torch.int32, device=dev)
    r = rows[perm]
    row16[:nnz] = torch.where(r >= 32768, r - 65536, r).to(torch.int16)
    perm32[:nnz] = perm.to(torch.int32)
    return col_ptr.to(torch.int32).contiguous(), row16, perm32


class SparseTrainStep:
    def __init__(self, cn, optimizer: FusedAdam, x: torch.Tensor, y: torch.Tensor, samples: int, sigma: float = 1.0,
                 prior=None, warmup: int = 2):
        """`cn`: a posthoc.CompressedNetwork; `optimizer`: FusedAdam(cn.parameters(), capturable=True); `x`, `y`: an example
        minibatch (shape / dtype of every later one); `prior`: an ops.PriorSpec (default: cn.prior, the source network's).
        The bias keep mask is taken once, here, from b_sigma != 0.  Building the object leaves the parameters, the moments,
        the step word and the sample counter as they were."""
        prior = cn.prior if prior is None else prior
        if prior is None:
            raise ops.BnnHipError("SparseTrainStep: no prior -- this CompressedNetwork records none (built by hand or from a "
                                  "state dict): pass prior=ops.PriorSpec(...)")
        if not all(g.get("capturable") for g in optimizer.param_groups):
            raise ops.BnnHipError("SparseTrainStep needs FusedAdam(capturable=True)")
        if state.host_eps:
            raise ops.BnnHipError("SparseTrainStep draws eps on chip; host/injected eps cannot be captured")
        if state.shard_samples:
            raise ops.BnnHipError("SparseTrainStep: shard MC samples outside the captured step")
        layers = cn._layers
        if len(layers) != 3:
            raise ops.BnnHipError("SparseTrainStep: a CompressedNetwork of three layers")
        keeps = [(c.b_sigma != 0) for c in layers]
        if sum(cn.nnz) == 0 and not any(bool(k.any()) for k in keeps):
            raise ops.BnnHipError("SparseTrainStep: the network has no survivor at all: nothing to train")
        if int(samples) < 1:
            raise ops.BnnHipError("SparseTrainStep: samples >= 1")
        ops.require_device(x, y, *[c.row_ptr for c in layers])
        self.cn, self.opt, self.samples, self.sigma, self.prior = cn, optimizer, int(samples), float(sigma), prior
        dev = x.device
        S = self.samples
        self.x, self.y = cn._x(x).clone(), y.clone()
        self.x16 = None                                        # exact fp32 throughout: no bf16 copy of the minibatch
        self.rows = rows = self.x.shape[0]
        self.beta = torch.zeros((), dtype=torch.float32, device=dev)
        sh = self._shared = SampleCounter.of(optimizer, dev)
        self.counter, self.base = sh["counter"], sh["base"]
        self.keep = [k.to(torch.uint8).contiguous() for k in keeps]            # owned by the step
        self.csc = [csc_view(c.row_ptr, c.col, c.nnz, c.fin) if i > 0 else (None, None, None) for i, c in enumerate(layers)]

        # ---- parameters and the flat gradient bucket (each slice 256-byte aligned); p.grad are views of it
        self.params = cn.parameters()
        self.bucket, offs = grad_bucket(self.params, dev, never_empty=True)
        self.grad_views = [self.bucket[o:o + p.numel()] for o, p in zip(offs, self.params)]
        self._grad_store = [self.bucket[o:o + max(p.numel(), 1)] for o, p in zip(offs, self.params)]   # (never an empty tensor)
        for p, g in zip(self.params, self.grad_views):
            p.grad = g if p.numel() else None                  # an empty layer's value arrays take no Adam slot

        # ---- static activations, gradients and argument blocks
        f = dict(dtype=torch.float32, device=dev)
        c1, c2, c3 = layers
        self.xt = torch.empty((c1.fin, rows), **f)
        self.h = [torch.empty((S, c1.fout, rows), **f), torch.empty((S, c2.fout, rows), **f)]
        self.logits = torch.empty((S, rows, c3.fout), **f)
        self.gh = [torch.empty((S, c1.fout, rows), **f), torch.empty((S, c2.fout, rows), **f)]
        self.log_prior, self.log_q, self.nll = (torch.empty(S, **f) for _ in range(3))
        first = self.base & 0xFFFFFFFF                         # + the shared device counter, added by every launch
        rnd = dict(seed=state.seed, sample_offset=first, sample_counter=self.counter)
        self._fwd = [ops.sparse_fwd_args(row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, sigma_val=c.sigma_val, b_mu=c.b_mu,
                                         b_sigma=c.b_sigma, x=xin, y=yout, n_samples=S, rows=rows, in_features=c.fin,
                                         out_features=c.fout, eps_mode=L.EPS_PHILOX, relu=relu, x_per_sample=xps,
                                         x_feature_major=xfm, y_feature_major=yfm, layer_id=c.layer_id, x_scratch=scr, **rnd)
                     for c, xin, yout, relu, xps, xfm, yfm, scr in ((c1, self.x, self.h[0], True, 0, False, True, self.xt),
                                                                    (c2, self.h[0], self.h[1], True, 1, True, True, None),
                                                                    (c3, self.h[1], self.logits, False, 1, True, False, None))]
        tl = [dict(row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, sigma_val=c.sigma_val, b_mu=c.b_mu, b_sigma=c.b_sigma, b_keep=k,
                   in_features=c.fin, out_features=c.fout, nnz=c.nnz, layer_id=c.layer_id) for c, k in zip(layers, self.keep)]
        self._terms = ops.sparse_elbo_terms_args(tl, n_samples=S, prior=prior, log_prior=self.log_prior, log_q=self.log_q,
                                                 workspace=ops.sparse_elbo_terms_workspace(tl, S, dev), **rnd)
        self._bwd_ws = ops.sparse_bwd_workspace(S, rows, max(c.fout for c in layers), dev)
        self._sigma = ops.sparse_sigma_args([(c.rho_val, c.sigma_val, None, c.nnz) for c in layers] +
                                            [(c.b_rho, c.b_sigma, k, c.fout) for c, k in zip(layers, self.keep)])
        self.out4, self.g_kl3 = torch.empty(4, **f), torch.empty(3, **f)
        self.g_lp, self.g_lq, self.g_logits = torch.empty(S, **f), torch.empty(S, **f), torch.empty_like(self.logits)
        tg, _ = ops._nll_target(self.y, cn.mode, rows, c3.fout)
        if tg.data_ptr() != self.y.data_ptr():
            raise ops.BnnHipError("SparseTrainStep: y must be contiguous int64 labels (classification) or float32 targets (regression)")
        self._rnd = rnd
        self._build_bwd()
        sh.sync()

        # ---- warm-up on a side stream, then undo its effects (the sigmas are the refresh launch's outputs)
        restore, mirror = snapshot(optimizer, extra=[t for c in layers for t in (c.sigma_val, c.b_sigma)]), sh["mirror"]
        warm_up(self._one_step, max(1, warmup))
        restore()
        sh.set(mirror)
        torch.cuda.synchronize()

        # ---- capture
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._one_step()

    # ------------------------------------------------------------------------------------------------ the launches
    def _chain(self):
        """terms -> forward x 3 -> finalize -> loss + seeds -> backward x 3: leaves the gradients in the bucket and returns
        (loss, mean log p, mean log q, nll) as views of the loss launch's out4."""
        cn, S = self.cn, self.samples
        ops.sparse_elbo_terms(self._terms)
        for a in self._fwd:
            ops.sparse_fwd(a)
        ops.elbo_finalize(workspaces=[], layer_in=[], layer_out=[], local_reparam=False, prior=self.prior, n_samples=S,
                          logits=self.logits, target=self.y, mode=cn.mode, nll_sigma=self.sigma, out=dict(nll=self.nll))
        self._loss()
        for a in self._bwd:
            ops.sparse_bwd(a)
        out4 = self.out4
        return out4[0:1], out4[1], out4[2], out4[3:4]

    def _loss(self):
        """bnn_elbo_loss_nll_bwd into the step's own buffers: out4, the seeds g_log_prior / g_log_q, g_logits."""
        ops.elbo_loss_nll_bwd(self.log_prior, self.log_q, self.nll, self.beta, self.samples, False, self.logits, self.y,
                              self.cn.mode, self.sigma, out=(self.out4, self.g_lp, self.g_lq, self.g_kl3, self.g_logits))

    def _build_bwd(self):
        g, g_a, g_b = self.g_logits, self.g_lp, self.g_lq
        c1, c2, c3 = self.cn._layers
        S, rows = self.samples, self.rows
        gv = self._grad_store
        # a hidden layer's ReLU mask is applied by the input-gradient launch of the layer above (its x IS that layer's output),
        # so no layer masks its own gy: (layer, x, x_per_sample, gy, y, relu, gy row-major, g_x, gx_relu_mask)
        spec = ((2, c3, self.h[1], 1, g, None, False, True, self.gh[1], True),
                (1, c2, self.h[0], 1, self.gh[1], None, False, False, self.gh[0], True),
                (0, c1, self.xt, 0, self.gh[0], None, False, False, None, False))
        self._bwd = []
        for i, c, xin, xps, gy, yy, relu, rowm, gx, mask in spec:
            cp, rw, pm = self.csc[i]
            self._bwd.append(ops.sparse_bwd_args(
                row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, rho_val=c.rho_val, b_mu=c.b_mu, b_rho=c.b_rho, b_keep=self.keep[i],
                x=xin, gy=gy, y=yy, g_mu_val=gv[4 * i], g_rho_val=gv[4 * i + 1], g_b_mu=gv[4 * i + 2], g_b_rho=gv[4 * i + 3],
                workspace=self._bwd_ws if (relu or rowm) else None, n_samples=S, rows=rows, in_features=c.fin, out_features=c.fout, nnz=c.nnz,
                prior=self.prior, relu=relu, gy_row_major=rowm, x_per_sample=xps, gx_relu_mask=mask, layer_id=c.layer_id,
                g_log_prior=g_a, g_log_q=g_b, g_x=gx, col_ptr=cp if gx is not None else None, row=rw if gx is not None else None,
                perm=pm if gx is not None else None, **self._rnd))

    def _update(self):
        with torch.no_grad():
            self.opt.bump_after_step(self.counter, self.samples)
            self.opt.step()
            ops.sparse_sigma_refresh(self._sigma)

    def _one_step(self):
        with torch.no_grad():
            out = self._chain()
        self._update()
        return out

    # ------------------------------------------------------------------------------------------------ the public step
    def step(self, x: torch.Tensor, y: torch.Tensor, beta: float):
        """One optimiser step on minibatch (x, y) with KL weight beta.  Returns (loss, mean log p, mean log q, nll): static
        tensors, read them before the next call."""
        x = x.reshape(self.x.shape) if x.numel() == self.x.numel() else x
        if (x.is_cuda and y.is_cuda and x.dtype == self.x.dtype and y.dtype == self.y.dtype and x.is_contiguous()
                and y.is_contiguous() and x.numel() == self.x.numel() and y.numel() == self.y.numel()):
            ops.stage_inputs(x, self.x, y, self.y, self.beta, float(beta))
        else:
            self.x.copy_(x, non_blocking=True)
            self.y.copy_(y, non_blocking=True)
            self.beta.fill_(float(beta))
        return self.replay()

    def replay(self):
        """The step on whatever the static buffers (x, y, beta) hold."""
        self.opt.sync_lr()
        self._shared.sync()
        self.graph.replay()
        self._shared.advance(self.samples)
        return self.out

    def eager(self):
        """The same launches issued one by one instead of replayed (bit for bit the replay's results): for tests and
        debugging.  Same bookkeeping as replay()."""
        self.opt.sync_lr()
        self._shared.sync()
        out = self._one_step()
        self._shared.advance(self.samples)
        return out
