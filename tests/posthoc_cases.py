"""Seeded inputs of the F3 / F4 fixture tests/golden/posthoc.npz: the recorder (oracle/make_golden_posthoc.py) runs the
real reference on them, the CPU and GPU tests regenerate them and check the sha256 the fixture holds.  Only
np.random.RandomState draws and plain arithmetic, so both sides build the same bytes."""
import hashlib

import numpy as np

DROPS = (0.0, 0.25, 0.5, 0.8, 0.95, 1.0)
BAND_DB = 3e-5                      # the SNR bound of tests/test_gpu_posthoc.py: the width of the threshold band
LAYERS = ("l1", "l2", "l3")
PARAMS = ("weight_mu", "weight_rho", "bias_mu", "bias_rho")


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ------------------------------------------------------------------------------------------------------------ ECE (G10)
def _simplex_rows(rs, n, C):
    """Flat Dirichlet draws on a random face of the simplex: the spacings of k - 1 sorted uniforms over k of the C
    classes (k in 2..C), exact zeros elsewhere, the classes rotated by a random shift.  k = 2 rows are uniform on
    (0, 1), so every confidence bin fills."""
    u = rs.random_sample((n, C - 1))
    k = rs.randint(2, C + 1, n)
    shift = rs.randint(0, C, n)
    u[np.arange(C - 1)[None, :] >= (k - 1)[:, None]] = 1.0
    u.sort(axis=1)
    cuts = np.concatenate([np.zeros((n, 1)), u, np.ones((n, 1))], axis=1)
    p = cuts[:, 1:] - cuts[:, :-1]
    idx = (np.arange(C)[None, :] + shift[:, None]) % C
    return np.take_along_axis(p, idx, axis=1).astype(np.float32)


def _labels(rs, p, right=0.7):
    n, C = p.shape
    return np.where(rs.random_sample(n) < right, p.argmax(1), rs.randint(0, C, n)).astype(np.int64)


def _random_case(n, C, seed, step=0.1, labels="mixed"):
    rs = np.random.RandomState(seed)
    p = _simplex_rows(rs, n, C)
    if labels == "mixed":
        y = _labels(rs, p)
    elif labels == "right":
        y = p.argmax(1).astype(np.int64)
    else:                                                    # every label wrong: every bin_corrects 0
        y = ((p.argmax(1) + 1) % C).astype(np.int64)
    return p, y, step, C


def _on_edge(step):
    """C = 2.  float32(k / 10) and its two fp32 neighbours for k = 0..10 (the bin edges are float64 k * 0.1: a kernel
    that compared against fp32 edges moves the on-edge value), the argmax ties (0.5, 0.5) under both labels, (0, 1) and
    (1, 0) (exact zeros fall out of the bins and of the total), 1 + 2^-23 (above the last edge: falls out), then 40
    filler rows so that every bin has both hits and misses."""
    first = []
    for k in range(11):
        c = np.float32(k / 10)
        first += [np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))]
    first = np.asarray(first, np.float32)
    assert first[-1] == np.float32(1 + 2.0 ** -23)
    rows = np.stack([first, (np.float32(1) - first).astype(np.float32)], axis=1)
    extra = np.asarray([[0.5, 0.5], [0.5, 0.5], [0.0, 1.0], [1.0, 0.0]], np.float32)
    rs = np.random.RandomState(1000 + int(round(step * 100)))
    f = rs.random_sample(40).astype(np.float32)
    fill = np.stack([f, (np.float32(1) - f).astype(np.float32)], axis=1)
    p = np.concatenate([rows, extra, fill]).astype(np.float32)
    y = _labels(rs, p, right=0.6)
    y[len(rows)], y[len(rows) + 1] = 0, 1                   # the ties: first-maximum argmax is class 0
    return p, y, step, 2


TIE_ROWS = (33, 34)                                         # the (0.5, 0.5) rows of an on-edge case


def _sparse(n, C, seed):
    """A few confident rows only: most bins stay empty (the reference's loop then walks off bin_acc)."""
    rs = np.random.RandomState(seed)
    p = np.full((n, C), 0.25 / (C - 1))
    p[np.arange(n), rs.randint(0, C, n)] = 0.75
    p = p.astype(np.float32)
    return p, _labels(rs, p), 0.1, C


# name -> (builder, compared on ece: every bin populated and the reference returns, inputs stored in the fixture)
ECE_CASES = {
    "baseline": (lambda: _random_case(10000, 10, 11), True, False),
    "edge_s10": (lambda: _on_edge(0.1), True, True),
    "edge_s20": (lambda: _on_edge(0.2), True, True),
    "edge_s25": (lambda: _on_edge(0.25), True, True),
    "edge_s50": (lambda: _on_edge(0.5), True, True),
    "n63": (lambda: _random_case(63, 2, 63), True, False),
    "n64": (lambda: _random_case(64, 3, 64), True, False),
    "n65": (lambda: _random_case(65, 2, 65), True, False),
    "n1023": (lambda: _random_case(1023, 3, 1023), True, False),
    "n1025": (lambda: _random_case(1025, 2, 1025), True, False),
    "n263169": (lambda: _random_case(262144 + 1025, 3, 263169), True, False),
    "c37": (lambda: _random_case(2000, 37, 37), True, False),
    "all_wrong": (lambda: _random_case(500, 10, 501, labels="wrong"), True, False),
    "all_right": (lambda: _random_case(500, 10, 502, labels="right"), True, False),
    "raise_n1": (lambda: _random_case(1, 10, 1), False, True),
    "raise_sparse": (lambda: _sparse(257, 37, 257), False, False),
    "raise_s05": (lambda: _random_case(2000, 10, 5, step=0.05), False, False),
}


def ece_case(name):
    """(probs float32 [n, C], labels int64 [n], bin_step, num_classes)."""
    return ECE_CASES[name][0]()


# ---------------------------------------------------------------------------------------------------- SNR / pruning (G11)
def _shapes(dims, lr):
    (i, h, o) = dims
    out = {}
    for l, (fin, fout) in zip(LAYERS, ((i, h), (h, h), (h, o))):
        out[l] = ((fin, fout) if lr else (fout, fin), (fout,))
    return out


def trained_like(dims, seed, lr=False):
    """A 12-key fp32 state dict with a trained network's spread: mu = N(0, 0.1) * exp(U(-6, 0)), rho = U(-9, 0.5)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for l, (ws, bs) in _shapes(dims, lr).items():
        for kind, shape in (("weight", ws), ("bias", bs)):
            mu = rs.standard_normal(shape) * 0.1 * np.exp(rs.uniform(-6.0, 0.0, shape))
            sd[f"{l}.{kind}_mu"] = mu.astype(np.float32)
            sd[f"{l}.{kind}_rho"] = rs.uniform(-9.0, 0.5, shape).astype(np.float32)
    return {f"{l}.{n}": sd[f"{l}.{n}"] for l in LAYERS for n in PARAMS}


# (tensor, flat index, mu or None, rho or None): never a pair that is NaN in either arithmetic (0 / 0, inf / inf)
EDGES = (
    ("l1.weight", 5, 0.0, None), ("l1.weight", 70, -0.0, None), ("l1.weight", 131, 1e-40, None),
    ("l1.weight", 258, -1e-40, -0.25), ("l1.weight", 300, np.inf, None), ("l1.weight", 421, None, 89.0),
    ("l1.weight", 555, None, -100.0), ("l2.weight", 9, -np.inf, None), ("l2.weight", 64, None, 89.0),
    ("l2.weight", 200, 1e-40, -8.5), ("l2.bias", 3, 0.0, None), ("l3.weight", 17, None, -100.0),
    ("l3.bias", 1, None, 89.0), ("l3.bias", 4, 1e-40, None),
)


def _poke(sd, pokes):
    for tensor, i, mu, rho in pokes:
        if mu is not None:
            sd[tensor + "_mu"].reshape(-1)[i] = np.float32(mu)
        if rho is not None:
            sd[tensor + "_rho"].reshape(-1)[i] = np.float32(rho)
    return sd


# name -> (dims, local_reparam, builder, stored whole in the fixture)
SNR_NETS = {
    "small": ((37, 19, 5), False, lambda: trained_like((37, 19, 5), 3705), True),
    "large": ((119, 100, 10), False, lambda: trained_like((119, 100, 10), 11910), False),
    "edges": ((37, 19, 5), False, lambda: _poke(trained_like((37, 19, 5), 3706), EDGES), True),
    "nan": ((37, 19, 5), False, lambda: _poke(trained_like((37, 19, 5), 3707),
                                                (("l1.weight", 11, np.nan, None), ("l2.bias", 2, None, np.nan))), True),
    "lr": ((37, 19, 5), True, lambda: trained_like((37, 19, 5), 3708, lr=True), True),
}


def snr_net(name):
    """(dims, local_reparam, 12-key fp32 state dict)."""
    dims, lr, build, _ = SNR_NETS[name]
    return dims, lr, build()


def state_hash(sd):
    return sha256(*[sd[f"{l}.{n}"] for l in LAYERS for n in PARAMS])


def flat12(sd):
    """The twelve tensors of a state dict as one flat fp32 array (l1.weight_mu, l1.weight_rho, l1.bias_mu, ...)."""
    return np.concatenate([np.asarray(sd[f"{l}.{n}"], np.float32).ravel() for l in LAYERS for n in PARAMS])


def unflat12(flat, dims, lr=False):
    sd, o = {}, 0
    for l, (ws, bs) in _shapes(dims, lr).items():
        for n in PARAMS:
            shape = ws if n.startswith("weight") else bs
            size = int(np.prod(shape))
            sd[f"{l}.{n}"] = flat[o:o + size].reshape(shape).copy()
            o += size
    assert o == flat.size
    return sd


def flat_order(sd, what):
    """The named_parameters() order of collect_weights: per layer weight then bias, flattened (`what`: 'mu' / 'rho')."""
    return np.concatenate([sd[f"{l}.{k}_{what}"].ravel() for l in LAYERS for k in ("weight", "bias")])


def band_differs(got_keep, ref_keep, snr64, thr, width):
    """The band rule: the positions where the two keep masks differ OUTSIDE the band |snr64 - thr| <= width (those must
    be none), and the number of elements in the band."""
    with np.errstate(invalid="ignore"):
        band = np.abs(snr64 - thr) <= width
    return np.flatnonzero((got_keep != ref_keep) & ~band), int(band.sum())
