"""What every captured object (train.GraphedTrainStep, dense_train.GraphedDenseTrainStep, sparse_train.SparseTrainStep, the
Laplace, MC-dropout, SG-MCMC and bandit graphs) needs around its launches, in one place: the uint32 word encoding, the
optimiser's shared device sample counter and its host mirror, the warm-up on a side stream and the undo of what it did to
the optimiser, the capture on a side stream, the flat gradient bucket.  Imports torch and runtime only (no kernel is
launched from here), so it loads without the library and runs on CPU tensors."""
from __future__ import annotations

import torch

from .runtime import state, take_samples


def word32(value: int) -> int:
    """The int32 a torch word stores for the uint32 `value` (the kernels read the word unsigned)."""
    value = int(value) & 0xFFFFFFFF
    return value - (1 << 32) if value >= (1 << 31) else value


class SampleCounter(dict):
    """ONE device MC-sample counter per optimiser (`optimizer._sample_words`), shared by every step object built on it (full
    batches and the 96-row last MNIST batch are two objects on one net): a step draws global sample index base + counter,
    the counter advances inside the captured step, so alternating objects never replay an index.  The words stay the dict
    they always were -- `counter` (device int32[1]), `base`, `mirror` (the host's copy of the device word) -- with the
    three operations on them as methods."""

    def __init__(self, device):
        super().__init__(counter=torch.zeros(1, dtype=torch.int32, device=device), base=take_samples(0), mirror=0)

    @classmethod
    def of(cls, optimizer, device) -> "SampleCounter":
        """The optimiser's counter; a new one when it has none yet or its word lives on another device."""
        sh = getattr(optimizer, "_sample_words", None)
        if sh is None or sh["counter"].device != device:
            sh = optimizer._sample_words = cls(device)
        return sh

    def set(self, value: int):
        self["mirror"] = value & 0xFFFFFFFF
        self["counter"].fill_(word32(self["mirror"]))

    def sync(self):
        """Before a step: the device counter must equal the host's count of indices drawn since `base` (eager evaluations
        between steps draw from the host counter); one small fill when they differ, nothing otherwise."""
        want = (state.counter - self["base"]) & 0xFFFFFFFF
        if want != self["mirror"]:
            self.set(want)

    def advance(self, n: int):
        """After a step whose launches added n to the device word: the host counter and the mirror follow."""
        take_samples(n)
        self["mirror"] = (self["mirror"] + n) & 0xFFFFFFFF


def warm_up(fn, n: int = 1, sync_first: bool = False):
    """fn() n times on a new side stream that waits for the current one (allocator pools, lazy inits); the current stream
    waits for it and the device is drained."""
    if sync_first:
        torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(n):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def snapshot(optimizer, extra=()):
    """Take down what a warm-up step changes -- the parameters, optimizer.state, every entry of every optimizer._dev[gi]
    (device step / learning-rate words, "last lr written", ticket, an SG-MCMC table and bank), the `extra` tensors and the
    host's state.counter -- and return restore(), which puts all of it back IN PLACE (a graph captured afterwards holds the
    addresses).  State the warm-up created is zeroed, as a fresh optimiser's; device words it created start from the
    host-side step."""
    params = [p for g in optimizer.param_groups for p in g["params"]]

    def copy(v):
        return v.clone() if torch.is_tensor(v) else v

    def put_back(holder, key, saved):
        if torch.is_tensor(saved) and torch.is_tensor(holder[key]):
            holder[key].copy_(saved)
        else:
            holder[key] = saved

    saved_p = [p.detach().clone() for p in params]
    saved_x = [t.clone() for t in extra]
    saved_state = {p: {k: copy(v) for k, v in optimizer.state[p].items()} for p in params if optimizer.state.get(p)}
    saved_dev = {gi: [copy(w) for w in d] for gi, d in getattr(optimizer, "_dev", {}).items()}
    host_counter = state.counter

    @torch.no_grad()
    def restore():
        state.counter = host_counter
        for t, s in zip(params + list(extra), saved_p + saved_x):
            t.copy_(s)
        for p in params:
            st = optimizer.state.get(p)
            if not st:
                continue
            if p in saved_state:
                for k, v in saved_state[p].items():
                    put_back(st, k, v)
            else:
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
        for gi, d in getattr(optimizer, "_dev", {}).items():
            if gi in saved_dev:
                # every entry: the learning-rate word and the "last lr written" beside it must stay a pair, or sync_lr()
                # takes a rate for written that the word no longer holds
                for i, s in enumerate(saved_dev[gi]):
                    put_back(d, i, s)
            elif d[0].dtype == torch.int32:                  # a step word (FusedSGD's first entry is its float32 rate)
                steps = [int(saved_state[p]["step"]) for p in optimizer.param_groups[gi]["params"]
                         if p in saved_state and "step" in saved_state[p]]
                d[0].fill_(max(steps) if steps else 0)

    return restore


def capture_on_side_stream(*fns, stream=None):
    """Capture each callable's launches as a hipGraph of its own, one after the other inside one region on a side stream
    (`stream`, or a new one) that waits for the current stream and that the current stream waits for afterwards.
    Returns the graph, or the tuple of graphs when several callables are given."""
    side = stream if stream is not None else torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs = []
    with torch.cuda.stream(side):
        for fn in fns:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append(g)
    torch.cuda.current_stream().wait_stream(side)
    return graphs[0] if len(fns) == 1 else tuple(graphs)


def grad_bucket(params, device, never_empty: bool = False):
    """(bucket, offsets): one zeroed flat fp32 gradient buffer and where each parameter's slice starts in it; every slice
    is a multiple of 64 elements, so each starts 256-byte aligned.  `never_empty`: a parameter of no elements still takes a
    slice (SparseTrainStep hands the kernels no empty tensor)."""
    offs, tot = [], 0
    for p in params:
        offs.append(tot)
        tot += (max(p.numel(), 1 if never_empty else 0) + 63) // 64 * 64
    return torch.zeros(tot, dtype=torch.float32, device=device), offs
