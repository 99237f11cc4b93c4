"""Generate tests/golden/posthoc.npz (groups G10, G11) by RUNNING THE REAL REFERENCE's compute_ece.py and
weight_pruning.py on the CPU of the build container.

TEST INFRASTRUCTURE, beside make_golden.py.  Both reference modules import plotting and data-loading packages at module
scope that are not installed here; only their plotting / loading code uses them.  Each such package is TRIED first and
gets an empty placeholder module (class Placeholder below, our own few lines) only when its import genuinely fails, so
that ECELoss, collect_weights, compute_snr and prune_weights run as the reference wrote them, against the reference's
own networks.BayesianNetwork.  Inputs come from tests/posthoc_cases.py; the fixture holds data only: per case the
sha256 of the input bytes and what the reference returned (or the class name of what it raised).

Run:    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_posthoc.py
Check:  PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_posthoc.py --check     (regenerate, compare array for array)
"""
from __future__ import annotations

import copy
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True


class Placeholder(types.ModuleType):
    """Stands in for a package that is not installed: any attribute is another placeholder, calling one is an error."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return Placeholder(f"{self.__name__}.{name}")

    def __call__(self, *a, **k):
        raise RuntimeError(f"{self.__name__} is a placeholder: the recorder never plots or loads data")


PLACED = []
for _name in ("matplotlib", "matplotlib.pyplot", "seaborn", "tqdm", "pandas", "sklearn", "torchvision",
              "torch.utils.tensorboard"):
    try:
        importlib.import_module(_name)
    except Exception:                       # genuinely fails when tried: only then the placeholder
        sys.modules[_name] = Placeholder(_name)
        PLACED.append(_name)

sys.path.insert(0, REF)
import networks as ref  # noqa: E402  (the real reference)
import compute_ece as ref_ece  # noqa: E402
import weight_pruning as ref_wp  # noqa: E402
sys.path.remove(REF)
while "../" in sys.path:                    # (classification/class_task.py appends it)
    sys.path.remove("../")
for _m in list(sys.modules):                # keep the reference's modules under private names only
    if _m.split(".")[0] in ("networks", "config", "utils", "classification", "compute_ece", "weight_pruning"):
        sys.modules.pop(_m, None)
for _m in PLACED:
    sys.modules.pop(_m, None)
sys.path.insert(0, os.path.join(REPO, "tests"))
import posthoc_cases as C  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "posthoc.npz")
MAX_BYTES = 256 * 1024
torch.set_num_threads(1)


# ------------------------------------------------------------------------------------------------------------------ G10
def g10(out):
    report = []
    for name, (_, compared, stored) in C.ECE_CASES.items():
        p, y, step, classes = C.ece_case(name)
        k = f"G10/{name}/"
        out[k + "sha256"] = C.sha256(p, y)
        out[k + "n"], out[k + "classes"], out[k + "step"] = np.int64(p.shape[0]), np.int64(classes), np.float64(step)
        if stored:
            out[k + "probs"], out[k + "labels"] = p, y
        crit = ref_ece.ECELoss(bin_step=step, num_classes=classes)
        raised = ""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                ece, centers, acc = crit(p, y)
            except Exception as e:          # recorded, not hidden: the class name goes into the fixture
                raised = type(e).__name__
        out[k + "raised"] = np.asarray(raised)
        if compared:
            assert not raised, (name, raised)
            n_bins = len(np.arange(0, 1.1, step)) - 1
            assert len(centers) == n_bins and len(acc) == n_bins, (name, "a bin is empty")
        else:
            assert raised, (name, "expected the reference to raise")
        if not raised:
            out[k + "ece"], out[k + "centers"], out[k + "bin_acc"] = np.float64(ece), np.asarray(centers, np.float64), np.asarray(acc, np.float64)
        report.append(f"  {name:13s} n={p.shape[0]:6d} C={classes:2d} step={step:<4} " + (f"raised {raised}" if raised else f"returned ece={ece:.6f}"))
    return report


# ------------------------------------------------------------------------------------------------------------------ G11
def make_net(dims, lr, sd):
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=8, hidden_units=dims[1], mode="classification",
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = ref.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return net.eval()


def state(net):
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def keep_mask(before, after):
    """Survivors of one prune_weights call in collect_weights order.  A pruned pair is (mu * 0, rho * 0); no generated
    rho is 0, so rho tells (NaN * 0 = NaN: such an entry is never a survivor, SNR NaN > threshold is False)."""
    rb, ra, ma = C.flat_order(before, "rho"), C.flat_order(after, "rho"), C.flat_order(after, "mu")
    assert not (rb == 0).any()
    return (ra != 0) & ~np.isnan(rb) & ~np.isnan(ma)


def g11(out):
    report = []
    for name, (dims, lr, _, stored) in C.SNR_NETS.items():
        _, _, sd = C.snr_net(name)
        k = f"G11/{name}/"
        out[k + "sha256"] = C.state_hash(sd)
        net = make_net(dims, lr, sd)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mus, sigmas = ref_wp.collect_weights(net, bnn=True)
            snr = [ref_wp.compute_snr(m, s) for m, s in zip(mus, sigmas)]            # weight_pruning.py main(): the float64 list
            thr = np.asarray([np.percentile(snr, 100 * d) for d in C.DROPS], np.float64)
        snr64 = np.asarray(snr, np.float64)
        assert snr64.size == sum(v.size for kk, v in sd.items() if kk.endswith("mu"))
        out[k + "thresholds"] = thr
        out[k + "snr_sha256"] = C.sha256(snr64)
        if stored:
            out[k + "in"] = C.flat12(sd)
            m32 = np.asarray(mus, np.float32)                                        # fp32 values in a python list: stored as fp32
            assert np.array_equal(m32.astype(np.float64), np.asarray(mus, np.float64), equal_nan=True)
            out[k + "mus"], out[k + "snr"] = m32, snr64
            if name in ("small", "edges"):
                out[k + "sigmas"] = np.asarray(sigmas, np.float64)
        # the reference's OWN fp32 arithmetic (weight_pruning.py:98-104 in torch), observed through prune_weights at the
        # threshold -1e300 (below every finite fp32 value): the survivors are the entries whose fp32 SNR is above -inf.  At rho = 89 the float64 list says
        # 10 log10(|mu| / 89) while torch's log1p(exp(89)) is +inf and the fp32 SNR -inf.
        probe = copy.deepcopy(net)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_wp.prune_weights(probe, [-1e300], 0.0)     # (np.percentile of [-inf] is NaN)
        after = state(probe)
        if lr:
            assert all(np.array_equal(after[kk].view(np.int32), sd[kk].view(np.int32)) for kk in sd)
        else:
            above = keep_mask(sd, after)
            out[k + "f32_above_neg_inf"] = np.packbits(above)
            rho = C.flat_order(sd, "rho")
            with np.errstate(invalid="ignore"):
                two_paths = np.isfinite(snr64) & ~above                              # finite in float64, -inf in fp32
            assert np.array_equal(two_paths, rho == 89.0), name                      # exactly the overflowing softplus
            # and the reference's own fp32 sigma (GaussianNode.sigma, networks.py:38-39): where it is +inf
            sig32 = torch.cat([node.sigma.detach().flatten() for l in net.children() if isinstance(l, ref.BayesianLinear)
                               for node in (l.weight, l.bias)]).numpy()
            assert np.array_equal(np.isinf(sig32), rho == 89.0), name
            out[k + "f32_sigma_inf"] = np.packbits(np.isinf(sig32))
        bands, kepts = [], []
        for di, d in enumerate(C.DROPS):
            c = copy.deepcopy(net)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref_wp.prune_weights(c, snr, drop_percentage=d)
            after = state(c)
            if lr:                          # isinstance(layer, BayesianLinear) is False for every layer: nothing is touched
                assert all(np.array_equal(after[kk].view(np.int32), sd[kk].view(np.int32)) for kk in sd)
                continue
            keep = keep_mask(sd, after)
            with np.errstate(invalid="ignore"):
                band = int((np.abs(snr64 - thr[di]) <= C.BAND_DB).sum())
            assert band <= max(1, snr64.size // 1000), (name, d, band)              # the band rule cannot hide a failure
            bands.append(band)
            kepts.append(int(keep.sum()))
            out[k + f"keep/{di}"] = np.packbits(keep)
            if stored and not (name == "nan" and di):                               # (the NaN network: six times the same)
                out[k + f"pruned/{di}"] = C.flat12(after)
            if name == "nan":
                assert not keep.any() and C.flat12(after).tobytes() == out[k + "pruned/0"].tobytes()
        out[k + "unchanged"] = np.int64(lr)
        if not lr:
            out[k + "band"], out[k + "kept"] = np.asarray(bands, np.int64), np.asarray(kepts, np.int64)
        fin = snr64[np.isfinite(snr64)]
        report.append(f"  {name:6s} {dims} lr={lr}: {snr64.size} SNRs in [{fin.min():.1f}, {fin.max():.1f}] dB, "
                      f"{int((~np.isfinite(snr64)).sum())} non-finite; thresholds {np.array2string(thr, precision=3)}; "
                      + ("left unchanged by prune_weights" if lr else f"band {bands} kept {kepts}"))
    return report


def build():
    out = {}
    report = ["G10 (ECELoss):"] + g10(out) + ["G11 (collect_weights / compute_snr / prune_weights):"] + g11(out)
    return out, report


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


if __name__ == "__main__":
    out, report = build()
    print("placeholders installed for:", ", ".join(PLACED) or "none")
    print("\n".join(report))
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        bad = sorted(set(old.keys()) ^ set(out.keys())) + [k for k in out if k in old.keys() and not same(old[k], out[k])]
        print("check:", "OK, %d arrays identical" % len(out) if not bad else "DIFFERENT: %s" % bad[:20])
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("posthoc.npz", len(out), "arrays,", size, "bytes")
    assert size < MAX_BYTES, size
