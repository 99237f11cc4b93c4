"""CPU-side checks of the grouped Thompson-sampling BNN bandits (include/bnn_hip.h F7, bnn_hip.bandit.BNNBanditGroup; no
GPU): the new entry points are exported and declared, the ctypes mirrors match the header, every argument check runs on
the host before a launch, and the Python refusals happen before the device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bnn_hip.h")
FAKE = 0x10000


def _layout(tmp_path, cls, cname, extra=()):
    lines = ['printf("%%zu\\n", sizeof(%s));' % cname]
    want = [C.sizeof(cls)]
    for fname, _t in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
        want.append(getattr(cls, fname).offset)
    for macro, value in extra:
        lines.append('printf("%%d\\n", %s);' % macro)
        want.append(value)
    prog = tmp_path / f"{cname}.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s return 0;}' % (HEADER, "".join(lines)))
    exe = tmp_path / cname
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == want


def test_bbb_group_exports_declarations_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    text = open(HEADER).read()
    for name in ("bnn_bbb_group_fwd", "bnn_bbb_group_train"):
        assert name in L.EXPORTS and hasattr(lib, name)
        assert f"int {name}(" in text
    assert "bnn_bbb_group_workspace_bytes" in L.EXPORTS and hasattr(lib, "bnn_bbb_group_workspace_bytes")
    assert "size_t bnn_bbb_group_workspace_bytes(" in text


def test_bbb_group_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.BbbGroupAgent, "bnn_bbb_group_agent")
    _layout(tmp_path, L.BbbGroupArgs, "bnn_bbb_group_args",
            [("BNN_BBB_GROUP_MAX_SAMPLES", L.BBB_GROUP_MAX_SAMPLES), ("BNN_MLP_GROUP_MAX_BATCHES", L.MLP_GROUP_MAX_BATCHES),
             ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    assert L.BBB_GROUP_MAX_SAMPLES >= 4                     # RLConfig draws 2


def test_bbb_group_workspace_query():
    from bnn_hip import _lib as L
    q = L.load().bnn_bbb_group_workspace_bytes
    P = 100 * 119 + 100 + 100 * 100 + 100 + 100 + 1        # the elements of a 119-100-100-1 network
    # the draw's weights, its eps and the two gradient accumulators, plus layer 1's weights a second time
    assert q(119, 100) >= 4 * (4 * P + 100 * 100) and q(119, 100) % 16 == 0
    assert q(119, 100) <= 4 * (4 * (P + 3) + 100 * 100 + 3) + 256
    assert q(1, 1) > 0 and q(L.MLP_GROUP_MAX_IN, L.MLP_GROUP_MAX_HIDDEN) > q(119, 100)
    for bad in ((0, 100), (119, 0), (L.MLP_GROUP_MAX_IN + 1, 100), (119, L.MLP_GROUP_MAX_HIDDEN + 1), (-1, -1)):
        assert q(*bad) == 0, bad


# ---------------------------------------------------------------------------------------------------- argument blocks
def _agent(train=True, **over):
    from bnn_hip import _lib as L
    a = L.BbbGroupAgent()
    for i in range(12):
        a.param[i] = FAKE
        if train:
            a.exp_avg[i], a.exp_avg_sq[i] = FAKE, FAKE
    fields = ("step", "lr", "slab", "targets", "n_batches", "loss_info", "sample_counter") if train else \
        ("rows", "outputs", "sample_counter")
    for f in fields + ("workspace",):
        setattr(a, f, FAKE)
    a.eps_seed, a.eps_mode = 2026, L.EPS_PHILOX
    for k, v in over.items():
        if k in ("param", "exp_avg", "exp_avg_sq"):
            i, v = v
            getattr(a, k)[i] = v
        else:
            setattr(a, k, v)
    return a


def _bbb(ags, prior=None, **over):
    from bnn_hip import _lib as L
    arr = (L.BbbGroupAgent * len(ags))(*ags)
    a = L.BbbGroupArgs()
    a.struct_bytes = C.sizeof(L.BbbGroupArgs)
    a.n_agents, a.in_features, a.hidden, a.out_features = len(ags), 119, 100, 1
    a.batch, a.max_batches, a.n_rows, a.n_samples = 64, 64, 2, 2
    a.prior = prior if prior is not None else L.Prior(L.PRIOR_MIXTURE, 1.0, 0.5, 1.0, 0.0025)
    a.beta1, a.beta2, a.eps, a.weight_decay = 0.9, 0.999, 1e-8, 0.0
    a.workspace_bytes = L.load().bnn_bbb_group_workspace_bytes(119, 100)
    a.agents_host, a.agents, a.agents_bytes = C.addressof(arr), FAKE, C.sizeof(arr)
    for k, v in over.items():
        setattr(a, k, v)
    a._keep = arr
    return a


SHARED_SHAPE = ("n_agents=0", "n_agents=-3", "n_agents=MAX_AGENTS+1", "in_features=0", "in_features=MAX_IN+1", "hidden=0",
                "hidden=MAX_HIDDEN+1", "out_features=2", "out_features=0", "n_samples=0", "n_samples=MAX_SAMPLES+1")


def _over(spec):
    from bnn_hip import _lib as L
    k, v = spec.split("=")
    names = dict(MAX_AGENTS=L.MLP_GROUP_MAX_AGENTS, MAX_IN=L.MLP_GROUP_MAX_IN, MAX_HIDDEN=L.MLP_GROUP_MAX_HIDDEN,
                 MAX_SAMPLES=L.BBB_GROUP_MAX_SAMPLES, MAX_BATCH=L.MLP_GROUP_MAX_BATCH, MAX_BATCHES=L.MLP_GROUP_MAX_BATCHES)
    if v.endswith("+1"):
        return {k: names[v[:-2]] + 1}
    return {k: int(v)}


def test_bbb_group_train_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_bbb_group_train
    assert fn(None, None) == -1
    assert fn(C.byref(_bbb([_agent()], struct_bytes=4)), None) == -5
    for spec in SHARED_SHAPE + ("batch=0", "batch=MAX_BATCH+1", "max_batches=0", "max_batches=MAX_BATCHES+1"):
        assert fn(C.byref(_bbb([_agent(), _agent()], **_over(spec))), None) == -2, spec
    for bad in (dict(beta1=1.0), dict(beta2=float("nan")), dict(eps=-1.0), dict(weight_decay=-0.5)):
        assert fn(C.byref(_bbb([_agent(), _agent()], **bad)), None) == -2, bad
    # the prior: an unknown kind, and scales that are not positive
    for kind in (2, -1, 7):
        assert fn(C.byref(_bbb([_agent()], prior=L.Prior(kind, 1.0, 0.5, 1.0, 0.0025))), None) == -3, kind
    assert fn(C.byref(_bbb([_agent()], prior=L.Prior(L.PRIOR_GAUSS, 0.0, 0.5, 1.0, 1.0))), None) == -2
    assert fn(C.byref(_bbb([_agent()], prior=L.Prior(L.PRIOR_MIXTURE, 1.0, 0.5, 1.0, 0.0))), None) == -2
    assert fn(C.byref(_bbb([_agent()], prior=L.Prior(L.PRIOR_MIXTURE, 1.0, 1.5, 1.0, 1.0))), None) == -2
    a = _bbb([_agent(), _agent()])
    a.agents_bytes = C.sizeof(L.BbbGroupAgent)                                   # the device copy holds one block, not two
    assert fn(C.byref(a), None) == -2
    assert fn(C.byref(_bbb([_agent()], n_agents=2)), None) == -2
    assert fn(C.byref(_bbb([_agent()], agents=None)), None) == -1
    assert fn(C.byref(_bbb([_agent()], agents_host=None)), None) == -1
    assert fn(C.byref(_bbb([_agent()], agents=FAKE + 4)), None) == -6
    # the workspace: too small for the shape, or missing in a block
    assert fn(C.byref(_bbb([_agent()], workspace_bytes=L.load().bnn_bbb_group_workspace_bytes(119, 100) - 1)), None) == -4
    assert fn(C.byref(_bbb([_agent()], workspace_bytes=0)), None) == -4
    assert fn(C.byref(_bbb([_agent(), _agent(workspace=None)])), None) == -4
    assert fn(C.byref(_bbb([_agent(workspace=FAKE + 8)])), None) == -6
    for f in ("step", "lr", "slab", "targets", "n_batches", "loss_info", "sample_counter"):
        assert fn(C.byref(_bbb([_agent(), _agent(**{f: None})])), None) == -1, f
    for f in ("param", "exp_avg", "exp_avg_sq"):
        assert fn(C.byref(_bbb([_agent(**{f: (7, None)})])), None) == -1, f
        assert fn(C.byref(_bbb([_agent(**{f: (11, FAKE + 2)})])), None) == -6, f
    assert fn(C.byref(_bbb([_agent(slab=FAKE + 1)])), None) == -6


def test_bbb_group_fwd_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_bbb_group_fwd
    assert fn(None, None) == -1
    assert fn(C.byref(_bbb([_agent(False)], struct_bytes=C.sizeof(L.BbbGroupArgs) - 8)), None) == -5
    for spec in SHARED_SHAPE + ("n_rows=0", "n_rows=MAX_BATCH+1"):
        assert fn(C.byref(_bbb([_agent(False)], **_over(spec))), None) == -2, spec
    assert fn(C.byref(_bbb([_agent(False), _agent(False)], agents_bytes=8)), None) == -2
    for f in ("rows", "outputs"):
        assert fn(C.byref(_bbb([_agent(False, **{f: None})])), None) == -1, f
    assert fn(C.byref(_bbb([_agent(False, param=(0, None))])), None) == -1
    assert fn(C.byref(_bbb([_agent(False, rows=FAKE + 2)])), None) == -6
    assert fn(C.byref(_bbb([_agent(False, workspace=None)])), None) == -4
    assert fn(C.byref(_bbb([_agent(False)], workspace_bytes=16)), None) == -4
    # the decision rule: a sampled forward needs the counter, the deterministic one does not; anything else is refused
    assert fn(C.byref(_bbb([_agent(False, sample_counter=None)])), None) == -1
    for mode in (L.EPS_MEMORY, 3, -1):
        assert fn(C.byref(_bbb([_agent(False), _agent(False, eps_mode=mode)])), None) == -3, mode


# ---------------------------------------------------------------------------------------------------- Python refusals
def _params(**over):
    p = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-3, hidden_units=100, mode="regression", epsilon=0.0,
             n_samples=2, mixture_prior=True, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6])
    p.update(over)
    return p


def _xy(N=50, d=117):
    rs = np.random.RandomState(0)
    return rs.uniform(0, 1, (N, d)).astype(np.float32), rs.randint(0, 2, N)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test with its own error, not a BnnHipError."""
    import torch

    def boom(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "current_device", boom)


@pytest.mark.parametrize("params,kw,match", [
    (_params(mode="classification"), {}, "regression"),
    (_params(), dict(local_reparam=True), "local reparameterisation"),
    (_params(local_reparam=True), {}, "local reparameterisation"),
    (_params(buffer_size=100), {}, "multiple"),
    (_params(hidden_units=129), {}, "limits"),
    (_params(batch_size=128, buffer_size=4096), {}, "limits"),
    (_params(batch_size=16, buffer_size=4096), {}, "limits"),               # 256 minibatches per update
    (_params(n_samples=0), {}, "limits"),
    (_params(n_samples=9), {}, "limits"),
    (_params(), dict(seeds=[]), "seeds"),
    (_params(), dict(epsilons=[0.0, float("nan")]), "epsilons"),
    (_params(), dict(epsilons=[1.5, 0.0]), "epsilons"),
    (_params(), dict(epsilons=[0.0]), "seeds"),
    (_params(), dict(eps_seeds=[1, 2, 3]), "seeds"),
    (_params(), dict(policy=["thompson"]), "seeds"),
    (_params(), dict(policy="greedy"), "policy"),
    (_params(lr=[1e-3, 1e-3, 1e-4]), {}, "seeds"),
    (_params(), dict(capture="graph"), "capture"),
])
def test_bnn_group_refusals_before_the_device(no_device, params, kw, match):
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    x, y = _xy()
    kw = dict(dict(seeds=[1, 2]), **kw)
    with pytest.raises(BnnHipError, match=match):
        bandit.BNNBanditGroup("g", params, x, y, **kw)


def test_bnn_group_refuses_a_context_beyond_the_input_limit(no_device):
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    x, y = _xy(d=127)                                                            # 127 + 2 > 128
    with pytest.raises(BnnHipError, match="limits"):
        bandit.BNNBanditGroup("g", _params(), x, y, seeds=[0])


def test_bnn_group_refuses_sample_sharding(no_device):
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    from bnn_hip.runtime import state
    x, y = _xy()
    old = state.shard_samples
    state.shard_samples = True
    try:
        with pytest.raises(BnnHipError, match="shard"):
            bandit.BNNBanditGroup("g", _params(), x, y, seeds=[0])
    finally:
        state.shard_samples = old


def test_kl_weight_table_is_the_references():
    """bandits.py:44 for the configured num_batches; the argument block holds it rounded once to fp32."""
    from bnn_hip import bandit
    nb = 64
    b = [bandit.beta(j, nb) for j in range(nb)]
    assert b[0] == 2.0 ** 63 / (2.0 ** 64 - 1) and abs(sum(b) - 1.0) < 1e-12
    assert all(np.float32(v) > 0 for v in b)                # down to 2^-64: still normal in fp32
