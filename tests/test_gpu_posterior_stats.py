"""F11 on an MI355X (bnn_param_hist, bnn_hip.diagnostics), through the C ABI and the Python API.  The transform is checked
through values_out against the kernels that already define it (bit for bit; the posterior sample to the one ulp a fused
multiply-add may differ from a twice-rounded one), the binning against numpy ON those materialised values (exact counts
and tallies; the fp64 sums to the worst-case reordering bound 2 n 2^-53 sum|terms| of two n-term sums), two calls are
bit-equal, and PosteriorStats / collect_weights equal the reference's host route (tests/posterior_stats_ref.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import posterior_stats_ref as R
import bnn_hip
from bnn_hip import _lib as L
from bnn_hip import diagnostics as D
from bnn_hip import ops, posthoc

SEED = 0x5EED0123456789AB
SIZES = (0, 1, 3, 10, 63, 64, 65, 4097)
MIXED = ((16, 8), (8,), (8, 8), (8,), (8, 3), (3,))                       # a 16-8-8-3 network's tensors
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _pack(arrays, dev, lead=1):
    """The arrays as views of ONE device buffer at odd element offsets: no start is 16-byte aligned relative to the others."""
    offs, pos = [], lead
    for i, a in enumerate(arrays):
        offs.append(pos)
        pos += a.size + 1 + i % 3
    flat = np.zeros(pos + 1, F32)
    for o, a in zip(offs, arrays):
        flat[o:o + a.size] = a.reshape(-1)
    buf = torch.from_numpy(flat).to(dev)
    views = [buf[o:o + a.size].view(a.shape) for o, a in zip(offs, arrays)]
    assert len({v.data_ptr() % 16 for v in views if v.numel()}) > 1 or len(arrays) < 2
    return views


def _records(a):
    """A call's records on the host: [dict per job]."""
    host = a.records.cpu().numpy()
    nb = int(a.n_edges) - 1
    out = []
    for row in host:
        head = row[nb:nb + 4].view(np.uint64)
        out.append(dict(counts=row[:nb].view(np.uint64).astype(np.int64), n_in=int(head[0]), n_below=int(head[1]),
                        n_above=int(head[2]), n_nan=int(head[3]), min=row[nb + 4:nb + 5].view(F32)[0],
                        max=row[nb + 4:nb + 5].view(F32)[1], sum=float(row[nb + 5:nb + 6].view(np.float64)[0]),
                        sum_sq=float(row[nb + 6:nb + 7].view(np.float64)[0])))
    return out


def _check_record(got, v, edges, what):
    """Exact against np.histogram on the materialised fp32 values; the sums to the reordering bound."""
    want = R.record(v, edges)
    print(what, "n", want["n"], "in/below/above/nan", got["n_in"], got["n_below"], got["n_above"], got["n_nan"],
          "sum err", abs(got["sum"] - want["sum"]), "sum_sq err", abs(got["sum_sq"] - want["sum_sq"]))
    assert np.array_equal(got["counts"], want["counts"]), what
    for f in ("n_in", "n_below", "n_above", "n_nan"):
        assert got[f] == want[f], (what, f)
    assert got["n_in"] + got["n_below"] + got["n_above"] + got["n_nan"] == want["n"], what
    assert got["min"] == want["min"] and got["max"] == want["max"], (what, got["min"], want["min"], got["max"], want["max"])
    n = want["n"]
    assert abs(got["sum"] - want["sum"]) <= 2 * n * 2.0 ** -53 * want["abs_sum"], what
    assert abs(got["sum_sq"] - want["sum_sq"]) <= 2 * n * 2.0 ** -53 * want["sum_sq"], what


def _run(jobs, edges, dev):
    """One call with a values_out per job (views of one buffer at odd offsets); returns (args, [values as numpy])."""
    outs = _pack([np.zeros(j["src0"].numel(), F32) for j in jobs], dev, lead=3)
    for j, o in zip(jobs, outs):
        j["values_out"] = o
    a = ops.param_hist_args(jobs, edges)
    ops.param_hist(a)
    torch.cuda.synchronize()
    return a, [o.cpu().numpy() for o in outs]


# ------------------------------------------------------------------------------------------------ 1. the transform
def _mu_rho(shape, rs):
    n = int(np.prod(shape))
    mu = (rs.standard_normal(n) * 0.1).astype(F32)
    rho = rs.uniform(-8.0, 3.0, n).astype(F32)
    mu[::7] = 0.0                                                          # SNR -inf
    mu[3::11] = -mu[3::11]
    return mu.reshape(shape), rho.reshape(shape)


def _sample_ref(mu, rho, tensor_id, sample, dev):
    """float32(float64(sigma) * float64(eps) + float64(mu)), sigma from bnn_softplus, eps from bnn_philox_normal."""
    rows, cols = (1, mu.numel()) if mu.dim() < 2 else (mu.shape[0], mu.shape[1])
    sig = ops.softplus(rho.contiguous()).cpu().numpy().astype(np.float64).reshape(-1)
    eps = ops.philox_normal(SEED, tensor_id, sample, 1, rows, cols, dev).cpu().numpy().astype(np.float64).reshape(-1)
    return (sig * eps + mu.cpu().numpy().astype(np.float64).reshape(-1)).astype(F32)


def _within_one_ulp(got, ref):
    up, down = np.nextafter(ref, F32(np.inf)), np.nextafter(ref, F32(-np.inf))
    return (got == ref) | (got == up) | (got == down)


def _transform_case(shapes, dev, seed):
    rs = np.random.RandomState(seed)
    pairs = [_mu_rho(s, rs) for s in shapes]
    mus = _pack([m for m, _ in pairs], dev, lead=1)
    rhos = _pack([r for _, r in pairs], dev, lead=2)
    return mus, rhos


@pytest.mark.parametrize("kind", ["value", "sigma", "snr_db", "sample"])
def test_transform_equals_its_defining_kernel(dev, kind):
    """values_out for every size, a multi-block tensor and 2-D shapes whose rows are no multiple of the epsilon group: VALUE
    is the source, SIGMA is bnn_softplus and SNR_DB is bnn_snr_db bit for bit (mu == 0 gives -inf, rho > 88 +inf); SAMPLE is
    within one fp32 ulp of the fp64 restatement (the product is exact in fp64, a fused and a twice-rounded result differ by
    at most one ulp)."""
    shapes = [(n,) for n in SIZES] + [(250, 281), (7, 13), (16, 8), (8, 3)]
    mus, rhos = _transform_case(shapes, dev, 11)
    if kind != "sample":
        rhos[-1].view(-1)[:2] = torch.tensor([89.0, -200.0], device=dev)  # exp overflows / underflows
    code = {"value": L.HIST_VALUE, "sigma": L.HIST_SIGMA, "snr_db": L.HIST_SNR_DB, "sample": L.HIST_SAMPLE}[kind]
    jobs = []
    for i, (m, r) in enumerate(zip(mus, rhos)):
        if kind == "value":
            jobs.append(dict(kind=code, src0=m))
        elif kind == "sigma":
            jobs.append(dict(kind=code, src0=r))
        else:
            jobs.append(dict(kind=code, src0=m, src1=r, seed=SEED, tensor_id=4 * (i % 3) + (m.dim() < 2), sample=5 + i))
    a, vals = _run(jobs, D.tensorboard_bins(), dev)
    for i, (m, r, v) in enumerate(zip(mus, rhos, vals)):
        if m.numel() == 0:
            assert v.size == 0
            continue
        mc, rc = m.contiguous().clone(), r.contiguous().clone()           # the defining kernels on aligned copies
        if kind == "value":
            assert np.array_equal(v.view(np.uint32), mc.cpu().numpy().reshape(-1).view(np.uint32))
        elif kind == "sigma":
            want = ops.softplus(rc).cpu().numpy().reshape(-1)
            assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), shapes[i]
        elif kind == "snr_db":
            want = ops.snr_db(mc, rc).cpu().numpy().reshape(-1)
            assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), shapes[i]
            assert np.isneginf(v[::7]).all()
        else:
            ref = _sample_ref(mc, rc, 4 * (i % 3) + (m.dim() < 2), 5 + i, dev)
            ok = _within_one_ulp(v, ref)
            print(shapes[i], "sample: differing by one ulp", int((v != ref).sum()), "of", v.size)
            assert ok.all(), (shapes[i], v[~ok][:4], ref[~ok][:4])
    if kind == "sigma":
        assert np.isposinf(vals[-1][0]) and vals[-1][1] == 0.0            # exp overflowed / underflowed, as the reference


# ------------------------------------------------------------------------------------------------ 2. the binning
def _tables():
    return {"two": np.array([-0.5, 0.5]), "three": np.array([-1.0, 0.0, 2.0]), "tensorboard": D.tensorboard_bins(),
            "uniform2048": D.uniform_bins(-8.0, -8.0 + 2047 / 128, 2047)}


def _values(n, edges, rs):
    """Normal values inside the table, then (for the first positions) values ON the first, last and interior edges, just
    outside both ends, +-inf, NaN and +-0."""
    scale = min(float(edges[-1] - edges[0]) / 4, 0.1 if edges.size > 1000 and edges[-1] > 1e6 else 4.0)
    v = (rs.standard_normal(n) * scale + (0.0 if edges[0] < 0 < edges[-1] else float(edges[0] + edges[-1]) / 2)).astype(F32)
    e32 = edges.astype(F32)
    special = [e32[0], e32[-1], e32[edges.size // 2], e32[1], e32[-2], np.nextafter(e32[0], F32(-np.inf)),
               np.nextafter(e32[-1], F32(np.inf)), F32(np.inf), F32(-np.inf), F32(np.nan), F32(0.0), F32(-0.0),
               e32[edges.size // 3], np.nextafter(e32[edges.size // 3], F32(-np.inf))]
    k = min(n, len(special))
    v[:k] = np.roll(np.array(special, F32), n)[:k]
    return v


@pytest.mark.parametrize("table", ["two", "three", "tensorboard", "uniform2048"])
def test_binning_equals_numpy_on_the_materialised_values(dev, table):
    """One call of eleven jobs at odd offsets: every size of SIZES, a tensor spanning several blocks (70 001 elements), one
    whose elements are all equal (the maximal collision in one bin) and one of values on every edge of the table; counts,
    tallies, min and max exact, the sums to the reordering bound; a second call returns the same bits."""
    edges = _tables()[table]
    if table == "uniform2048":
        assert edges.size == 2048 and np.array_equal(edges, edges.astype(F32).astype(np.float64))   # fp32 can sit ON every edge
    rs = np.random.RandomState(len(table))
    arrays = [_values(n, edges, rs) for n in SIZES] + [_values(70001, edges, rs), np.full(5000, 0.25, F32),
                                                      np.concatenate([edges.astype(F32), edges.astype(F32)[::-1]])]
    srcs = _pack(arrays, dev)
    a, vals = _run([dict(kind=L.HIST_VALUE, src0=s) for s in srcs], edges, dev)
    first = a.records.clone()
    for i, (arr, v, rec) in enumerate(zip(arrays, vals, _records(a))):
        assert np.array_equal(v.view(np.uint32), arr.view(np.uint32))
        _check_record(rec, v, edges, (table, i, arr.size))
    empty = _records(a)[0]
    assert empty["min"] == np.inf and empty["max"] == -np.inf and empty["sum"] == 0.0 and empty["sum_sq"] == 0.0
    assert empty["counts"].sum() == 0 and empty["n_in"] == empty["n_nan"] == 0
    ops.param_hist(a)
    torch.cuda.synchronize()
    assert torch.equal(first, a.records)                                   # bit-equal, the fp64 sums included


def test_twelve_mixed_jobs_in_one_call(dev):
    """The twelve tensors of a 16-8-8-3 network (16x8, 8, 8x8, 8, 8x3, 3, and the same again) with the four kinds mixed in
    one call, sliced from one buffer at odd offsets: each record equals numpy on its own values, each values_out its
    defining kernel (SAMPLE: one ulp)."""
    mus, rhos = _transform_case(MIXED + MIXED, dev, 5)
    kinds = [L.HIST_VALUE, L.HIST_SIGMA, L.HIST_SNR_DB, L.HIST_SAMPLE, L.HIST_SIGMA, L.HIST_SNR_DB,
             L.HIST_SAMPLE, L.HIST_VALUE, L.HIST_SAMPLE, L.HIST_SNR_DB, L.HIST_VALUE, L.HIST_SIGMA]
    jobs = []
    for i, (m, r, k) in enumerate(zip(mus, rhos, kinds)):
        jobs.append(dict(kind=k, src0=r if k == L.HIST_SIGMA else m, src1=r, seed=SEED, tensor_id=4 * (i // 2 % 3) + (m.dim() < 2),
                         sample=9))
    edges = D.tensorboard_bins()
    a, vals = _run(jobs, edges, dev)
    assert a.n_jobs == 12
    for i, (m, r, k, v, rec) in enumerate(zip(mus, rhos, kinds, vals, _records(a))):
        mc, rc = m.contiguous().clone(), r.contiguous().clone()
        if k == L.HIST_SAMPLE:
            assert _within_one_ulp(v, _sample_ref(mc, rc, 4 * (i // 2 % 3) + (m.dim() < 2), 9, dev)).all(), i
        else:
            want = {L.HIST_VALUE: lambda: mc, L.HIST_SIGMA: lambda: ops.softplus(rc), L.HIST_SNR_DB: lambda: ops.snr_db(mc, rc)}[k]()
            assert np.array_equal(v.view(np.uint32), want.cpu().numpy().reshape(-1).view(np.uint32)), i
        _check_record(rec, v, edges, ("mixed", i))


# ------------------------------------------------------------------------------------------------ 3. the Python level
def _net(dev, local_reparam):
    import networks
    torch.manual_seed(3 + int(local_reparam))
    net = networks.BayesianNetwork({'input_shape': 16, 'classes': 3, 'batch_size': 4, 'hidden_units': 8, 'mode': 'classification',
                                    'mu_init': [-0.2, 0.2], 'rho_init': [-5, -4], 'prior_init': [1.0], 'mixture_prior': False,
                                    'local_reparam': local_reparam}).to(dev)
    with torch.no_grad():
        net.l2.weight_mu.view(-1)[:3] = 0.0                                # SNR -inf: below every table
    return net


def _host_params(net):
    """{"l1.weight_mu": ndarray, ..., "l1.weight_sigma": ndarray}: the tensors write_weight_histograms hands to add_histogram.
    sigma is the project's fp32 softplus (bnn_softplus, which test 1 ties the kernel to bit for bit): the reference's
    torch.log1p(torch.exp(rho)) may differ from it in the last place, which could move a value across a 1.1-ratio edge."""
    out = {}
    for n, p in net.named_parameters():
        out[n] = p.detach().cpu().numpy()
        if n.endswith("_rho"):
            out[n[:-4] + "_sigma"] = ops.softplus(p.detach().contiguous()).cpu().numpy()
    return out


@pytest.mark.parametrize("local_reparam", [False, True])
def test_posterior_stats_equals_the_reference_route(dev, local_reparam):
    """read() per tag against write_weight_histograms' route (.cpu(), np.histogram over default_bins, make_histogram's
    trimming): counts, limits, num, min, max; the moments against numpy; SNR tags over uniform bins with cdf(tag)[-1] ==
    n_in / num and a density that integrates to one; posterior samples equal collect_weights' draw."""
    bnn_hip.manual_seed(SEED)
    net = _net(dev, local_reparam)
    ps = D.PosteriorStats(net, snr_bins=D.uniform_bins(-60.0, 40.0, 40))
    got = ps.update().read()
    torch.cuda.synchronize()
    want = R.weight_histograms(_host_params(net), D.tensorboard_bins())
    assert tuple(t for t in got if t.startswith("histogram/")) == R.TAGS == tuple(want)
    params = _host_params(net)
    for tag in R.TAGS:
        g, w = got[tag], want[tag]
        assert g["bucket_counts"] == w["bucket_counts"] and g["bucket_limits"] == w["bucket_limits"], tag
        assert g["num"] == w["num"] and g["min"] == w["min"] and g["max"] == w["max"], tag
        assert len(g["bucket_counts"]) == len(g["bucket_limits"]) and sum(g["bucket_counts"]) == g["num"]
    v = params["l1.weight_sigma"].reshape(-1).astype(np.float64)
    g = got["histogram/w1_rho"]
    assert abs(g["sum"] - v.sum()) <= 2 * v.size * 2.0 ** -53 * np.abs(v).sum()
    assert abs(g["sum_squares"] - (v * v).sum()) <= 2 * v.size * 2.0 ** -53 * (v * v).sum()
    snr_tags = [t for t in got if t.startswith("snr/")]
    assert snr_tags == [f"snr/{p}{i}" for p in "wb" for i in (1, 2, 3)]
    for tag in snr_tags:
        r = ps.raw(tag)
        l = getattr(net, "l" + tag[-1])
        mu, rho = (l.weight_mu, l.weight_rho) if tag[4] == "w" else (l.bias_mu, l.bias_rho)
        snr = ops.snr_db(mu.detach().contiguous(), rho.detach().contiguous()).cpu().numpy().reshape(-1)
        _check_record(r, snr, r["edges"], tag)
        cdf = ps.cdf(tag)
        assert cdf[-1] == r["n_in"] / r["num"] and np.all(np.diff(cdf) >= 0) and len(cdf) == 40
        centres, dens = ps.density(tag)
        assert len(centres) == 40 and abs(float((dens * np.diff(r["edges"])).sum()) - 1.0) <= 40 * 2.0 ** -52
    assert ps.raw("snr/w2")["n_below"] >= 3 and ps.cdf("snr/w2")[-1] < 1.0
    # one posterior draw per (mu, rho) tensor, at global sample index 4
    got = ps.update(sample=4).read()
    drawn = posthoc.collect_weights(net, bnn=True, sample=4).cpu().numpy()
    pos = 0
    for l, lname in ((net.l1, "1"), (net.l2, "2"), (net.l3, "3")):
        for p, t in ((l.weight_mu, "w"), (l.bias_mu, "b")):
            _check_record(ps.raw(f"sample/{t}{lname}"), drawn[pos:pos + p.numel()], D.tensorboard_bins(), f"sample/{t}{lname}")
            ref = _sample_ref(p.detach(), getattr(l, ("weight" if t == "w" else "bias") + "_rho").detach(),
                                     4 * (int(lname) - 1) + (t == "b"), 4, dev)
            assert _within_one_ulp(drawn[pos:pos + p.numel()], ref).all(), (t, lname)
            pos += p.numel()
    assert pos == drawn.size


def test_posterior_stats_of_a_plain_module(dev):
    """Any module: VALUE jobs over its parameters, so nn.Linear weights too."""
    torch.manual_seed(1)
    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 2)).to(dev)
    got = D.PosteriorStats(m).update().read()
    assert list(got) == [f"histogram/{n}" for n, _ in m.named_parameters()]
    for n, p in m.named_parameters():
        v = p.detach().cpu().numpy().reshape(-1)
        c, l = R.trim(*np.histogram(v.astype(np.float64), bins=D.tensorboard_bins()))
        g = got[f"histogram/{n}"]
        assert g["bucket_counts"] == c.tolist() and g["bucket_limits"] == l.tolist() and g["num"] == v.size
        assert g["min"] == float(v.min()) and g["max"] == float(v.max())


@pytest.mark.parametrize("local_reparam", [False, True])
def test_collect_weights_equals_the_reference_lists(dev, local_reparam):
    """mus exactly; sigmas against the reference's np.log(1 + np.exp(rho)) on python floats to 2^-20 relative: for rho in
    [-5, -4] the fp32 softplus carries the rounding of rho log2(e) (<= 5 x 2^-24 of exp(rho)), one ulp (2 x 2^-24) each of
    the hardware exp2 and log2, and two roundings of the final fma -- under 12 x 2^-24; 16 x 2^-24 = 2^-20 bounds it."""
    net = _net(dev, local_reparam)
    named = [(n, p.detach().cpu().numpy()) for n, p in net.named_parameters()]
    ref_mus, ref_sigmas = R.collect_weights(named, bnn=True)
    mus, sigmas = posthoc.collect_weights(net, bnn=True)
    assert mus.is_cuda and sigmas.is_cuda and mus.dtype == sigmas.dtype == torch.float32
    assert mus.cpu().numpy().astype(np.float64).tolist() == ref_mus
    s, r = sigmas.cpu().numpy().astype(np.float64), np.array(ref_sigmas)
    print("sigma: max relative error", float(np.max(np.abs(s - r) / r)))
    assert s.shape == r.shape and np.all(np.abs(s - r) <= 2.0 ** -20 * r)
    plain = torch.nn.Linear(4, 3).to(dev)
    w = posthoc.collect_weights(plain)
    assert w.cpu().numpy().astype(np.float64).tolist() == R.collect_weights([(n, p.detach().cpu().numpy()) for n, p in plain.named_parameters()])


def test_update_is_capturable_and_follows_the_parameters(dev):
    """update() captured in a torch.cuda.graph, replayed after a parameter change: read() reflects the new parameters."""
    net = _net(dev, False)
    ps = D.PosteriorStats(net)
    ps.update()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ps.update()
    with torch.no_grad():
        net.l1.weight_mu.mul_(3.0).add_(0.5)
        net.l3.bias_rho.fill_(-2.0)
    g.replay()
    torch.cuda.synchronize()
    got = ps.read()
    want = R.weight_histograms(_host_params(net), D.tensorboard_bins())
    for tag in R.TAGS:
        assert got[tag]["bucket_counts"] == want[tag]["bucket_counts"] and got[tag]["bucket_limits"] == want[tag]["bucket_limits"], tag
        assert got[tag]["min"] == want[tag]["min"] and got[tag]["max"] == want[tag]["max"], tag
    assert got["histogram/b3_rho"]["bucket_counts"] == [0, 3]              # three equal sigmas in one bin
