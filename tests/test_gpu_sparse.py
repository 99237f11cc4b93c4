"""The F13 compressed network on an MI355X (bnn_sparse_count, bnn_sparse_fill, bnn_sparse_fwd; posthoc.CompressedNetwork):
the CSR arrays exactly against the restatement of tests/test_sparse_cpu.py, one layer through the C ABI within the derived
fma-chain bound (chain_bound, same file) under every epsilon mode, the whole network against the fp64 restatement and the
sweep's masked forward, bitwise independence of batch cuts / sample counts / repeats, graph capture, and the summaries."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import _lib as L, ops, posthoc, synth
from oracle import bnn_oracle as O
from test_sparse_cpu import chain_bound_layer, csr_ref, sparse_forward_ref, sparse_layer_ref

LEVELS = (0., .5, .98, 1.)
NETS = [((1, 48, 1), "regression"), ((70, 130, 10), "classification"), ((119, 100, 1), "regression")]
FWD_TOL = 1e-5                                  # of the output scale: the f32 bound of tests/test_gpu_prune_sweep.py
PHILOX_ATOL = 5e-5                              # tests/test_gpu_parity.py
SEED = 2026


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _math_back():
    yield
    bnn_hip.set_math("bf16")


_cache = {}
_oracle = {}


def _oracle_eps(tensor_id, sample, rows, cols):
    key = (tensor_id, sample, rows, cols)
    if key not in _oracle:
        _oracle[key] = np.asarray(O.philox_normal(SEED, tensor_id, sample, rows, cols))
    return _oracle[key]


def _case(dims, mode, lr, dev):
    """(net, sweep over LEVELS, [CompressedNetwork per level]) -- built once and shared, never written."""
    key = (dims, lr)
    if key not in _cache:
        import networks
        mp = dict(input_shape=dims[0], classes=dims[2], batch_size=128, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
                  rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
        net = networks.BayesianNetwork(mp)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*dims, lr).items()})
        net = net.to(dev).eval()
        bnn_hip.set_math("f32")
        sweep = posthoc.PruneSweep(net, LEVELS)
        _cache[key] = (net, sweep, [sweep.compress(i) for i in range(len(LEVELS))])
    return _cache[key]


def _canonical(net):
    """Per layer the fp32 (W_mu, W_rho) in the canonical [out, in] layout and (b_mu, b_rho), numpy."""
    lr = bool(net.local_reparam)
    out = []
    for l in (net.l1, net.l2, net.l3):
        wm, wr = l.weight_mu.detach().cpu().numpy(), l.weight_rho.detach().cpu().numpy()
        out.append(((wm.T, wr.T) if lr else (wm, wr), (l.bias_mu.detach().cpu().numpy(), l.bias_rho.detach().cpu().numpy())))
    return out


def _ref_layers(net, sweep, i):
    """The restated CSR layers of level i: csr_ref over the sweep's codes, the original fp32 parameters gathered at the
    kept positions, sigma from the device's own softplus (the bits every kernel uses)."""
    rank = sweep.level_rank[i]
    layers = []
    for (wc, bc), ((wm, wr), (bm, br)), l in zip(sweep.codes(), _canonical(net), (net.l1, net.l2, net.l3)):
        wc, bc = wc.cpu().numpy(), bc.cpu().numpy()
        rp, col, rows = csr_ref(wc, rank)
        sig = ops.softplus(l.weight_rho.detach()).cpu().numpy()
        sig = sig.T if net.local_reparam else sig
        bsig = ops.softplus(l.bias_rho.detach()).cpu().numpy()
        keep = bc > rank
        layers.append(dict(row_ptr=rp, col=col, rows=rows, mu_val=wm[rows, col], rho_val=wr[rows, col], sigma_val=sig[rows, col],
                           b_mu=np.where(keep, bm, 0).astype(np.float32), b_sigma=np.where(keep, bsig, 0).astype(np.float32),
                           fin=wm.shape[1], fout=wm.shape[0]))
    return layers


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------- 1. CSR, exact
@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("dims,mode", NETS)
def test_csr_equals_the_restatement_and_to_dense_equals_prune_weights(dev, dims, mode, lr):
    net, sweep, cns = _case(dims, mode, lr, dev)
    for i, p in enumerate(LEVELS):
        cn = cns[i]
        ref = _ref_layers(net, sweep, i)
        for c, r in zip(cn._layers, ref):
            assert c.nnz == int(r["row_ptr"][-1]) and (c.fin, c.fout) == (r["fin"], r["fout"])
            np.testing.assert_array_equal(c.row_ptr.cpu().numpy(), r["row_ptr"])
            np.testing.assert_array_equal(_u16(c.col)[:c.nnz], r["col"])
            for name in ("mu_val", "rho_val", "sigma_val"):                        # fp32 copies / bnn_softplus' bits: exact
                np.testing.assert_array_equal(getattr(c, name).cpu().numpy()[:c.nnz].view(np.int32), r[name].view(np.int32), err_msg=name)
            np.testing.assert_array_equal(c.b_mu.cpu().numpy(), r["b_mu"])
            np.testing.assert_array_equal(c.b_sigma.cpu().numpy(), r["b_sigma"])
        assert cn.nnz == tuple(int(r["row_ptr"][-1]) for r in ref)
        assert cn.state_bytes == sum(t.numel() * t.element_size() for t in cn.state_dict().values())
        assert cn.state_bytes == posthoc.compressed_state_bytes([(r["fin"], r["fout"]) for r in ref], cn.nnz, True)
        pruned = copy.deepcopy(net)
        posthoc.prune_weights(pruned, None, p)
        want, got = pruned.state_dict(), cn.to_dense()
        assert sorted(got) == sorted(want) and len(got) == 12
        for k in want:
            assert got[k].shape == want[k].shape and torch.equal(_bits(got[k]), _bits(want[k])), (p, k)   # signed zeros included
        if p == 1.:
            assert cn.nnz == (0, 0, 0) and cn.density == 0.0
    light = sweep.compress(1, zero_signs=False)                                   # without the sign bits: equal in value
    pruned = copy.deepcopy(net)
    posthoc.prune_weights(pruned, None, LEVELS[1])
    for k, v in pruned.state_dict().items():
        assert torch.equal(light.to_dense()[k], v), k
    assert light.state_bytes < cns[1].state_bytes


@pytest.mark.parametrize("lr", [False, True])
def test_an_empty_row_among_full_ones(dev, lr):
    """100 of the 22 201 parameters -- one row of layer 2 -- are near zero; dropping the lowest 0.5 % removes that row and
    about eleven other entries: an empty row between nearly full ones."""
    net = copy.deepcopy(_case((119, 100, 1), "regression", lr, dev)[0])
    with torch.no_grad():
        tiny = 1e-12 * (1 + torch.arange(100, device=dev, dtype=torch.float32))
        if lr:
            net.l2.weight_mu[:, 5] = tiny
        else:
            net.l2.weight_mu[5, :] = tiny
    bnn_hip.set_math("f32")
    sweep = posthoc.PruneSweep(net, (0.005,))
    cn = sweep.compress(0)
    ref = _ref_layers(net, sweep, 0)
    rp = cn._layers[1].row_ptr.cpu().numpy()
    np.testing.assert_array_equal(rp, ref[1]["row_ptr"])
    assert rp[6] == rp[5] and (np.diff(rp) >= 95).sum() >= 98
    x_np, _ = synth.synth_batch("regression", 37, 119, 1, seed=3)
    got = cn.forward(torch.from_numpy(x_np).to(dev)).double().cpu().numpy()
    want = sparse_forward_ref(ref, x_np)
    assert np.abs(got - want).max() <= FWD_TOL * np.abs(want).max()


# ------------------------------------------------------------------------------------------------- 2. one layer, C ABI
def _layer_tensors(c):
    return dict(row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, sigma_val=c.sigma_val, b_mu=c.b_mu, b_sigma=c.b_sigma,
                in_features=c.fin, out_features=c.fout, layer_id=c.layer_id)


@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("dims,mode,li", [((70, 130, 10), "classification", 0), ((70, 130, 10), "classification", 1),
                                          ((119, 100, 1), "regression", 0), ((1, 48, 1), "regression", 2)])
def test_one_layer_within_the_chain_bound_in_every_epsilon_mode(dev, dims, mode, li, lr):
    net, sweep, cns = _case(dims, mode, lr, dev)
    rs = np.random.RandomState(dims[0] + li)
    for i, p in enumerate(LEVELS):
        c, r = cns[i]._layers[li], _ref_layers(net, sweep, i)[li]
        for rows, S, off in ((1, 1, 0), (37, 3, 5), (130, 1, 2)):
            x_np = rs.uniform(-1, 1, (rows, c.fin)).astype(np.float32)
            x = torch.from_numpy(x_np).to(dev)
            f = dict(dtype=torch.float32, device=dev)
            common = dict(x=x, n_samples=S, rows=rows, relu=False, **_layer_tensors(c))
            # the posterior mean
            y0 = torch.full((S, rows, c.fout), float("nan"), **f)
            ops.sparse_fwd(ops.sparse_fwd_args(y=y0, eps_mode=L.EPS_ZERO, **common))
            ref, w, b = sparse_layer_ref(r, x_np)
            bound = chain_bound_layer(x_np, r["row_ptr"], r["col"], w, b)
            err = np.abs(y0.double().cpu().numpy() - ref)
            print(f"layer {dims} l{li + 1} lr={lr} p={p} rows={rows}: mean-forward err / bound max {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= bound)
            # Philox, with the epsilon it used
            y1 = torch.full((S, rows, c.fout), float("nan"), **f)
            dump = torch.full((S, max(c.nnz, 1)), float("nan"), **f)
            dump_b = torch.full((S, c.fout), float("nan"), **f)
            scratch = torch.empty((c.fin, rows), **f)
            ops.sparse_fwd(ops.sparse_fwd_args(y=y1, eps_mode=L.EPS_PHILOX, seed=SEED, sample_offset=off, eps_dump=dump,
                                               eps_b_dump=dump_b, x_scratch=scratch, **common))
            dense = ops.philox_normal(SEED, 4 * c.layer_id + 0, off, S, c.fout, c.fin, dev).cpu().numpy()
            dense_b = ops.philox_normal(SEED, 4 * c.layer_id + 1, off, S, 1, c.fout, dev).cpu().numpy()[:, 0]
            e, eb = dump.cpu().numpy()[:, :c.nnz], dump_b.cpu().numpy()
            np.testing.assert_array_equal(e.view(np.int32), dense[:, r["rows"], r["col"].astype(np.int64)].view(np.int32))
            np.testing.assert_array_equal(eb.view(np.int32), dense_b.view(np.int32))
            y1n = y1.double().cpu().numpy()
            for s in range(S):
                orc = _oracle_eps(4 * c.layer_id, off + s, c.fout, c.fin)
                np.testing.assert_allclose(e[s], orc[r["rows"], r["col"].astype(np.int64)], atol=PHILOX_ATOL)
                np.testing.assert_allclose(eb[s], _oracle_eps(4 * c.layer_id + 1, off + s, 1, c.fout)[0], atol=PHILOX_ATOL)
                ref, w, b = sparse_layer_ref(r, x_np, (e[s], eb[s]))
                assert np.all(np.abs(y1n[s] - ref) <= chain_bound_layer(x_np, r["row_ptr"], r["col"], w, b))
            # the same epsilon from memory: the same bits
            y2 = torch.full((S, rows, c.fout), float("nan"), **f)
            ops.sparse_fwd(ops.sparse_fwd_args(y=y2, eps_mode=L.EPS_MEMORY, eps=dump, eps_b=dump_b, **common))
            assert torch.equal(_bits(y2), _bits(y1))
            # feature-major in and out, ReLU: the same chains
            y3 = torch.full((S, c.fout, rows), float("nan"), **f)
            ops.sparse_fwd(ops.sparse_fwd_args(y=y3, eps_mode=L.EPS_MEMORY, eps=dump, eps_b=dump_b, y_feature_major=True,
                                               **dict(common, x=x.t().contiguous(), x_feature_major=True, relu=True)))
            assert torch.equal(_bits(y3.transpose(1, 2)), _bits(torch.relu(y1)))


# ------------------------------------------------------------------------------------------------- 3. whole network
@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("dims,mode", NETS)
def test_forward_against_fp64_and_the_sweep(dev, dims, mode, lr):
    net, sweep, cns = _case(dims, mode, lr, dev)
    bnn_hip.set_math("f32")
    for rows in (1, 37, 130):
        x_np, _ = synth.synth_batch(mode, rows, dims[0], dims[2], seed=77)
        x = torch.from_numpy(x_np).to(dev)
        dense = sweep.forward(x).double().cpu().numpy()                           # [P, rows, classes], the masked MFMA forward
        for i, p in enumerate(LEVELS):
            got32 = cns[i].forward(x).clone()
            assert tuple(got32.shape) == (rows, dims[2]) and got32.dtype == torch.float32
            got = got32.double().cpu().numpy()
            ref = sparse_forward_ref(_ref_layers(net, sweep, i), x_np)
            scale = max(np.abs(ref).max(), 1e-30)
            err = np.abs(got - ref).max()
            print(f"forward {dims} lr={lr} rows={rows} p={p}: err {err:.3e} scale {scale:.3e}; bit-equal to the sweep: "
                  f"{np.array_equal(got, dense[i])}; max |sparse - sweep| {np.abs(got - dense[i]).max():.3e}")
            assert err <= FWD_TOL * scale
            if p == 1.:                                                           # nothing survives: exactly zero on both paths
                assert not got.any() and not dense[i].any() and not ref.any()     # (no margin to speak of: every logit ties)
                continue
            if mode == "classification":
                top = np.sort(ref, axis=1)
                clear = (top[:, -1] - top[:, -2]) > 2 * FWD_TOL * scale
                assert clear.mean() >= 0.9                                        # from the reference alone
                assert np.array_equal(got.argmax(1)[clear], ref.argmax(1)[clear])
                assert np.array_equal(got.argmax(1)[clear], dense[i].argmax(1)[clear])
                y = ref.argmax(1)                                                 # any labels: the counts agree where the margin is clear
                assert int((got.argmax(1)[clear] == y[clear]).sum()) == int((dense[i].argmax(1)[clear] == y[clear]).sum())


def test_evaluate_counts_equal_the_sweeps(dev):
    net, sweep, cns = _case((70, 130, 10), "classification", False, dev)
    bnn_hip.set_math("f32")
    xs, ys = zip(*[synth.synth_batch("classification", 100, 70, 10, seed=40 + i) for i in range(3)])
    X, Y = torch.from_numpy(np.concatenate(xs)).to(dev), torch.from_numpy(np.concatenate(ys)).to(dev)
    want = sweep.evaluate((X, Y), batch_size=128)
    for i in (1, 2):
        r = cns[i].evaluate((X, Y), batch_size=128)                              # 128 + 128 + 44 rows
        ref = sparse_forward_ref(_ref_layers(net, sweep, i), X.cpu().numpy())
        top = np.sort(ref, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2 * FWD_TOL * np.abs(ref).max()
        assert clear.all()                                                        # so the two paths must count alike
        assert r.total == 300 and int(r.correct[0]) == int(want.correct[i])
        np.testing.assert_allclose(r.nll[0], want.nll[i], rtol=2e-5)
        np.testing.assert_allclose(r.probs[0].cpu().numpy(), want.probs[i].cpu().numpy(), atol=1e-5)


# ------------------------------------------------------------------------------------------------- 4. order independence
@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("dims,mode", NETS)
def test_results_do_not_depend_on_batch_cuts_sample_counts_or_repeats(dev, dims, mode, lr):
    _, _, cns = _case(dims, mode, lr, dev)
    x_np, _ = synth.synth_batch(mode, 130, dims[0], dims[2], seed=9)
    x = torch.from_numpy(x_np).to(dev).reshape(130, dims[0])
    for cn in cns[:3]:
        whole = cn.forward(x).clone()
        parts = torch.cat([cn.forward(x[:64]).clone(), cn.forward(x[64:]).clone()])
        assert torch.equal(_bits(whole), _bits(parts))
        assert torch.equal(_bits(cn.forward(x)), _bits(whole))                    # a repeat
        mc = cn.forward_mc(x, 3, seed=SEED, sample_offset=0).clone()
        assert tuple(mc.shape) == (3, 130, dims[2])
        cut = torch.cat([cn.forward_mc(x[:64], 3, seed=SEED, sample_offset=0).clone(),
                         cn.forward_mc(x[64:], 3, seed=SEED, sample_offset=0).clone()], dim=1)
        assert torch.equal(_bits(mc), _bits(cut))
        singles = torch.cat([cn.forward_mc(x, 1, seed=SEED, sample_offset=s).clone() for s in range(3)])
        assert torch.equal(_bits(mc), _bits(singles))
        assert torch.equal(_bits(cn.forward_mc(x, 3, seed=SEED, sample_offset=0)), _bits(mc))
        if cn is cns[0]:
            assert not torch.equal(mc[0], mc[1])                                  # and the samples do differ


# ------------------------------------------------------------------------------------------------- 5. capture
def test_forward_mc_replays_with_a_device_sample_counter(dev):
    _, _, cns = _case((70, 130, 10), "classification", True, dev)
    cn = cns[1]
    x_np, _ = synth.synth_batch("classification", 37, 70, 10, seed=4)
    x = torch.from_numpy(x_np).to(dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    cn.forward_mc(x, 3, seed=SEED, sample_offset=0, sample_counter=counter)      # the first call for the shape allocates
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):                              # one stream, no parallel branches
            out = cn.forward_mc(x, 3, seed=SEED, sample_offset=0, sample_counter=counter)
    replays = []
    for k in range(3):
        counter.fill_(3 * k)
        graph.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    for k in range(3):
        eager = cn.forward_mc(x, 3, seed=SEED, sample_offset=3 * k).clone()
        assert torch.equal(_bits(replays[k]), _bits(eager)), k
    assert not torch.equal(replays[0], replays[1])


# ------------------------------------------------------------------------------------------------- 6. summaries, state
@pytest.mark.parametrize("dims,mode", [((70, 130, 10), "classification"), ((119, 100, 1), "regression")])
def test_summaries_and_the_state_dict_round_trip(dev, dims, mode):
    net, sweep, cns = _case(dims, mode, False, dev)
    cn = cns[1]
    x_np, y_np = synth.synth_batch(mode, 37, dims[0], dims[2], seed=6)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    kw = dict(seed=SEED, sample_offset=7)
    logits = cn.forward_mc(x, 3, **kw).clone()
    q = (0.05, 0.95) if mode == "regression" else None
    got = cn.predictive(x, 3, quantiles=q, sigma=0.5, **kw)
    want = ops.mc_predictive(logits, mode, sigma=0.5, quantiles=q or ())
    for name, a, b in zip(got._fields, got, want):
        if b is None:
            assert a is None
        else:
            b = b[:, 0] if name == "quantiles" else b[0]
            assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                      b.view(torch.int32) if b.dtype == torch.float32 else b), name
    s_got, s_want = cn.score(x, y, 3, sigma=0.5, **kw), ops.mc_score(logits, y, mode, sigma=0.5)
    assert torch.equal(s_got.record.view(torch.int64), s_want.record.view(torch.int64))
    if mode == "classification":
        preds, probs = cn.predict_mc(x, 3, **kw)
        assert torch.equal(preds, want.preds[0]) and torch.equal(_bits(probs), _bits(want.probs[0]))
    other = sweep.compress(2)                                                     # another level, then this one's state
    assert other.nnz != cn.nnz
    other.load_state_dict({k: v.clone() for k, v in cn.state_dict().items()})
    assert other.nnz == cn.nnz and other.state_bytes == cn.state_bytes
    assert torch.equal(_bits(other.forward(x)), _bits(cn.forward(x)))
    assert torch.equal(_bits(other.forward_mc(x, 3, **kw)), _bits(logits))
    for k, v in cn.to_dense().items():
        assert torch.equal(_bits(other.to_dense()[k]), _bits(v)), k


def test_one_level_compress_equals_the_sweeps_level(dev):
    net, sweep, cns = _case((70, 130, 10), "classification", False, dev)
    bnn_hip.set_math("f32")
    cn = posthoc.compress(net, 0.5)
    assert cn.nnz == cns[1].nnz and cn.drop_percentage == 0.5
    for k, v in cns[1].state_dict().items():
        assert torch.equal(cn.state_dict()[k], v), k
