"""CPU-side checks of the grouped epsilon-greedy MLP bandits (include/bnn_hip.h F6, bnn_hip.bandit.GreedyBanditGroup; no
GPU): the new entry points are exported and declared, the ctypes mirrors match the header, every argument check runs on
the host before a launch, and the Python refusals happen before the device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bnn_hip.h")
ENTRIES = ("bnn_bandit_rows_group", "bnn_bandit_act_group", "bnn_bandit_replay_group", "bnn_mlp_group_fwd",
           "bnn_mlp_group_train")
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


def test_group_exports_declarations_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    text = open(HEADER).read()
    for name in ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert f"int {name}(" in text


def test_group_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.BanditGroupArgs, "bnn_bandit_group_args")
    _layout(tmp_path, L.MlpGroupAgent, "bnn_mlp_group_agent")
    _layout(tmp_path, L.MlpGroupArgs, "bnn_mlp_group_args",
            [("BNN_MLP_GROUP_MAX_IN", L.MLP_GROUP_MAX_IN), ("BNN_MLP_GROUP_MAX_HIDDEN", L.MLP_GROUP_MAX_HIDDEN),
             ("BNN_MLP_GROUP_MAX_OUT", L.MLP_GROUP_MAX_OUT), ("BNN_MLP_GROUP_MAX_BATCH", L.MLP_GROUP_MAX_BATCH),
             ("BNN_MLP_GROUP_MAX_BATCHES", L.MLP_GROUP_MAX_BATCHES), ("BNN_MLP_GROUP_MAX_AGENTS", L.MLP_GROUP_MAX_AGENTS),
             ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    # RLConfig's shape is inside the limits: input 117 + 2, hidden 100, output 1, batch 64, 4096 / 64 minibatches
    assert L.MLP_GROUP_MAX_IN >= 119 and L.MLP_GROUP_MAX_HIDDEN >= 100 and L.MLP_GROUP_MAX_BATCH >= 64
    assert L.MLP_GROUP_MAX_BATCHES >= 64 and L.MLP_GROUP_MAX_OUT == 1


# ---------------------------------------------------------------------------------------------------- argument blocks
def _act_block(**over):
    from bnn_hip import _lib as L
    a = L.BanditActArgs()
    a.struct_bytes = C.sizeof(L.BanditActArgs)
    a.n_actions, a.n_labels, a.n_samples, a.output_sample_stride = 2, 2, 1, 0
    a.context_dim, a.n_contexts, a.buffer_size, a.max_steps, a.epsilon = 10, 100, 32, 40, 0.0
    for f in ("x", "labels", "rewards", "oracle", "outputs", "step", "cur_index", "rows", "actions", "reward_out", "regrets",
              "counts", "ring_index", "ring_action", "ring_reward"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _replay_block(**over):
    from bnn_hip import _lib as L
    a = L.BanditReplayArgs()
    a.struct_bytes = C.sizeof(L.BanditReplayArgs)
    a.batch_size, a.num_batches, a.buffer_size, a.context_dim, a.n_actions, a.n_contexts = 8, 4, 32, 10, 2, 100
    for f in ("step", "x", "ring_index", "ring_action", "ring_reward", "workspace", "slab", "targets"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _group(blks, **over):
    """(args, keep-alive): host array of the blocks; the device copy is a fake, never dereferenced address."""
    from bnn_hip import _lib as L
    arr = (type(blks[0]) * len(blks))(*blks)
    g = L.BanditGroupArgs()
    g.struct_bytes = C.sizeof(L.BanditGroupArgs)
    g.n_agents, g.blocks_host, g.blocks, g.blocks_bytes = len(blks), C.addressof(arr), FAKE, C.sizeof(arr)
    for k, v in over.items():
        setattr(g, k, v)
    g._keep = arr
    return g, arr


@pytest.mark.parametrize("entry", ["bnn_bandit_rows_group", "bnn_bandit_act_group"])
def test_act_group_validation_without_a_device(entry):
    from bnn_hip import _lib as L
    fn = getattr(L.load(), entry)
    assert fn(None, None) == -1
    g, keep = _group([_act_block(), _act_block(epsilon=0.05)])
    assert fn(C.byref(_group([_act_block()], struct_bytes=8)[0]), None) == -5          # BNN_ERR_ABI
    for over in (dict(n_agents=0), dict(n_agents=-1), dict(n_agents=L.MLP_GROUP_MAX_AGENTS + 1)):
        assert fn(C.byref(_group([_act_block()], **over)[0]), None) == -2, over
    # the device copy's size must be the host blocks': a mismatched block count is refused
    g, keep = _group([_act_block(), _act_block()])
    g.blocks_bytes = C.sizeof(L.BanditActArgs)
    assert fn(C.byref(g), None) == -2
    g, keep = _group([_act_block(), _act_block()], n_agents=3)
    g.blocks_bytes = 2 * C.sizeof(L.BanditActArgs)
    assert fn(C.byref(g), None) == -2
    assert fn(C.byref(_group([_act_block()], blocks=None)[0]), None) == -1
    assert fn(C.byref(_group([_act_block()], blocks_host=None)[0]), None) == -1
    assert fn(C.byref(_group([_act_block()], blocks=FAKE + 4)[0]), None) == -6
    # every block is checked with F5's rules: a bad second agent is caught
    for bad in (dict(epsilon=float("nan")), dict(epsilon=-0.1), dict(epsilon=1.5), dict(n_actions=1), dict(buffer_size=0)):
        assert fn(C.byref(_group([_act_block(), _act_block(**bad)])[0]), None) == -2, bad
    assert fn(C.byref(_group([_act_block(), _act_block(rows=None)])[0]), None) == -1
    assert fn(C.byref(_group([_act_block(struct_bytes=4), _act_block()])[0]), None) == -5


def test_replay_group_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_bandit_replay_group
    assert fn(None, None) == -1
    assert fn(C.byref(_group([_replay_block()], n_agents=0)[0]), None) == -2
    g, keep = _group([_replay_block(), _replay_block()])
    g.blocks_bytes = 3 * C.sizeof(L.BanditReplayArgs)
    assert fn(C.byref(g), None) == -2
    for bad in (dict(buffer_size=36), dict(batch_size=0), dict(num_batches=3), dict(n_actions=1)):   # 36 % 8: not a multiple
        assert fn(C.byref(_group([_replay_block(), _replay_block(**bad)])[0]), None) == -2, bad
    assert fn(C.byref(_group([_replay_block(slab=None)])[0]), None) == -1
    assert fn(C.byref(_group([_replay_block(targets=FAKE + 2)])[0]), None) == -6


def _agent(train=True, **over):
    from bnn_hip import _lib as L
    a = L.MlpGroupAgent()
    for i in range(6):
        a.param[i] = FAKE
        if train:
            a.exp_avg[i], a.exp_avg_sq[i] = FAKE, FAKE
    fields = ("step", "lr", "slab", "targets", "n_batches", "loss") if train else ("rows", "outputs")
    for f in fields:
        setattr(a, f, FAKE)
    for k, v in over.items():
        if k in ("param", "exp_avg", "exp_avg_sq"):
            i, v = v
            getattr(a, k)[i] = v
        else:
            setattr(a, k, v)
    return a


def _mlp(ags, **over):
    from bnn_hip import _lib as L
    arr = (L.MlpGroupAgent * len(ags))(*ags)
    a = L.MlpGroupArgs()
    a.struct_bytes = C.sizeof(L.MlpGroupArgs)
    a.n_agents, a.in_features, a.hidden, a.out_features = len(ags), 119, 100, 1
    a.batch, a.max_batches, a.n_rows = 64, 64, 2
    a.beta1, a.beta2, a.eps, a.weight_decay = 0.9, 0.999, 1e-8, 0.0
    a.agents_host, a.agents, a.agents_bytes = C.addressof(arr), FAKE, C.sizeof(arr)
    for k, v in over.items():
        setattr(a, k, v)
    a._keep = arr
    return a


def test_mlp_group_train_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_mlp_group_train
    assert fn(None, None) == -1
    assert fn(C.byref(_mlp([_agent()], struct_bytes=4)), None) == -5
    for bad in (dict(n_agents=0), dict(n_agents=-3), dict(in_features=0), dict(in_features=L.MLP_GROUP_MAX_IN + 1),
                dict(hidden=0), dict(hidden=L.MLP_GROUP_MAX_HIDDEN + 1), dict(out_features=2), dict(out_features=0),
                dict(batch=0), dict(batch=L.MLP_GROUP_MAX_BATCH + 1), dict(max_batches=0),
                dict(max_batches=L.MLP_GROUP_MAX_BATCHES + 1), dict(beta1=1.0), dict(beta2=float("nan")), dict(eps=-1.0),
                dict(weight_decay=-0.5)):
        assert fn(C.byref(_mlp([_agent(), _agent()], **bad)), None) == -2, bad
    a = _mlp([_agent(), _agent()])
    a.agents_bytes = C.sizeof(L.MlpGroupAgent)                                   # the device copy holds one block, not two
    assert fn(C.byref(a), None) == -2
    assert fn(C.byref(_mlp([_agent()], n_agents=2)), None) == -2
    assert fn(C.byref(_mlp([_agent()], agents=None)), None) == -1
    assert fn(C.byref(_mlp([_agent()], agents_host=None)), None) == -1
    assert fn(C.byref(_mlp([_agent()], agents=FAKE + 4)), None) == -6
    for f in ("step", "lr", "slab", "targets", "n_batches", "loss"):
        assert fn(C.byref(_mlp([_agent(), _agent(**{f: None})])), None) == -1, f
    for f in ("param", "exp_avg", "exp_avg_sq"):
        assert fn(C.byref(_mlp([_agent(**{f: (3, None)})])), None) == -1, f
        assert fn(C.byref(_mlp([_agent(**{f: (5, FAKE + 2)})])), None) == -6, f
    assert fn(C.byref(_mlp([_agent(slab=FAKE + 1)])), None) == -6


def test_mlp_group_fwd_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_mlp_group_fwd
    assert fn(None, None) == -1
    for bad in (dict(n_rows=0), dict(n_rows=L.MLP_GROUP_MAX_BATCH + 1), dict(in_features=L.MLP_GROUP_MAX_IN + 1),
                dict(hidden=0), dict(out_features=3), dict(n_agents=0)):
        assert fn(C.byref(_mlp([_agent(False)], **bad)), None) == -2, bad
    assert fn(C.byref(_mlp([_agent(False), _agent(False)], agents_bytes=8)), None) == -2
    for f in ("rows", "outputs"):
        assert fn(C.byref(_mlp([_agent(False, **{f: None})])), None) == -1, f
    assert fn(C.byref(_mlp([_agent(False, param=(0, None))])), None) == -1
    assert fn(C.byref(_mlp([_agent(False, rows=FAKE + 2)])), None) == -6


# ---------------------------------------------------------------------------------------------------- Python refusals
def _params(**over):
    p = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-3, hidden_units=100, mode="regression", epsilon=0.0,
             n_samples=1)
    p.update(over)
    return p


def _xy(N=50, d=117):
    rs = np.random.RandomState(0)
    return rs.uniform(0, 1, (N, d)).astype(np.float32), rs.randint(0, 2, N)


@pytest.mark.parametrize("params,kw,match", [
    (_params(mode="classification"), {}, "regression"),
    (_params(buffer_size=100), {}, "multiple"),
    (_params(hidden_units=129), {}, "limits"),
    (_params(batch_size=128, buffer_size=4096), {}, "limits"),
    (_params(batch_size=16, buffer_size=4096), {}, "limits"),               # 256 minibatches per update
    (_params(), dict(epsilons=[0.0, float("nan")]), "epsilons"),
    (_params(), dict(epsilons=[1.5]), "epsilons"),
    (_params(), dict(epsilons=[-0.01]), "epsilons"),
    (_params(), dict(epsilons=[]), "epsilons"),
    (_params(), dict(epsilons=[0.0, 0.05], seeds=[1]), "seeds"),
])
def test_group_refusals_before_the_device(params, kw, match):
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    x, y = _xy()
    kw = dict(dict(epsilons=[0.0, 0.01]), **kw)
    with pytest.raises(BnnHipError, match=match):
        bandit.GreedyBanditGroup("g", params, x, y, **kw)


def test_group_refuses_a_context_beyond_the_input_limit():
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    x, y = _xy(d=127)                                                            # 127 + 2 > 128
    with pytest.raises(BnnHipError, match="limits"):
        bandit.GreedyBanditGroup("g", _params(), x, y, epsilons=[0.0])
    with pytest.raises(BnnHipError, match="limits"):
        bandit.GreedyBandit("g", _params(), x, y)


def test_group_refuses_sample_sharding():
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    from bnn_hip.runtime import state
    x, y = _xy()
    old = state.shard_samples
    state.shard_samples = True
    try:
        with pytest.raises(BnnHipError, match="shard"):
            bandit.GreedyBanditGroup("g", _params(), x, y, epsilons=[0.0])
    finally:
        state.shard_samples = old


def test_greedy_bandit_takes_epsilon_from_its_parameters():
    from bnn_hip import bandit
    from bnn_hip.ops import BnnHipError
    x, y = _xy()
    with pytest.raises(BnnHipError, match="epsilons"):
        bandit.GreedyBandit("g", _params(epsilon=2.0), x, y)
