"""CPU-side checks of the device contextual bandit (bnn_bandit_rows / _act / _replay, bnn_hip.bandit; no GPU): the ctypes
mirrors of the argument structs match the header, every argument check runs on the host before a launch, and the host's
schedule (nb(t), beta_j, the replay pool of each regime) restates base_bandit.py:77-84."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bnn_hip.h")


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


def test_bandit_exports_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in ("bnn_bandit_rows", "bnn_bandit_act", "bnn_bandit_replay"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_bandit_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.BanditActArgs, "bnn_bandit_act_args",
            [("BNN_BANDIT_MAX_ACTIONS", L.BANDIT_MAX_ACTIONS), ("BNN_BANDIT_MAX_BUFFER", L.BANDIT_MAX_BUFFER),
             ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.BanditReplayArgs, "bnn_bandit_replay_args")


FAKE = 0x10000


def _act_args(**over):
    from bnn_hip import _lib as L
    a = L.BanditActArgs()
    a.struct_bytes = C.sizeof(L.BanditActArgs)
    a.n_actions, a.n_labels, a.n_samples, a.output_sample_stride = 2, 2, 2, 2
    a.context_dim, a.n_contexts, a.buffer_size, a.max_steps, a.epsilon = 10, 100, 32, 40, 0.0
    for f in ("x", "labels", "rewards", "oracle", "outputs", "step", "cur_index", "rows", "actions", "reward_out", "regrets",
              "counts", "ring_index", "ring_action", "ring_reward"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _replay_args(**over):
    from bnn_hip import _lib as L
    a = L.BanditReplayArgs()
    a.struct_bytes = C.sizeof(L.BanditReplayArgs)
    a.batch_size, a.num_batches, a.buffer_size, a.context_dim, a.n_actions, a.n_contexts = 8, 4, 32, 10, 2, 100
    for f in ("step", "x", "ring_index", "ring_action", "ring_reward", "workspace", "slab", "targets"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("entry", ["bnn_bandit_rows", "bnn_bandit_act"])
def test_act_argument_validation_without_a_device(entry):
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    fn = getattr(L.load(), entry)
    assert fn(None, None) == -1                                                   # BNN_ERR_NULL
    assert fn(C.byref(_act_args(struct_bytes=C.sizeof(L.BanditActArgs) - 8)), None) == -5   # BNN_ERR_ABI
    for bad in (dict(n_actions=1), dict(n_actions=65), dict(n_labels=0), dict(n_samples=0), dict(output_sample_stride=1),
                dict(buffer_size=8193), dict(buffer_size=0), dict(context_dim=0), dict(n_contexts=0), dict(max_steps=0),
                dict(epsilon=float("nan")), dict(epsilon=1.5)):
        assert fn(C.byref(_act_args(**bad)), None) == -2, bad                    # BNN_ERR_SHAPE
    for f in ("x", "labels", "rewards", "oracle", "outputs", "step", "cur_index", "rows", "actions", "regrets", "counts",
              "ring_index", "ring_action", "ring_reward"):
        assert fn(C.byref(_act_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_act_args(n_indices=5)), None) == -1                        # a sequence without its pointer
    assert fn(C.byref(_act_args(regrets=FAKE + 4)), None) == -6                   # BNN_ERR_ALIGN (fp64)


def test_replay_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_bandit_replay
    assert fn(None, None) == -1
    assert fn(C.byref(_replay_args(struct_bytes=C.sizeof(L.BanditReplayArgs) + 8)), None) == -5
    for bad in (dict(buffer_size=36), dict(buffer_size=8192 + 8, num_batches=2000), dict(n_actions=1), dict(batch_size=0),
                dict(num_batches=3), dict(context_dim=0), dict(n_contexts=0)):
        assert fn(C.byref(_replay_args(**bad)), None) == -2, bad
    for f in ("step", "x", "ring_index", "ring_action", "ring_reward", "workspace", "slab", "targets"):
        assert fn(C.byref(_replay_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_replay_args(slab=FAKE + 2)), None) == -6


def _reference_pool(l, bs, buffer_size):
    """base_bandit.py:77-82 verbatim, without the permutation: the buffer indices the pool draws from."""
    if l <= bs:
        idx_pool = int(bs // l + 1) * list(range(l))
        return idx_pool[-bs:]
    elif l > bs and l < buffer_size:
        idx_pool = int(l // bs) * bs
        return list(range(l))[-idx_pool:]
    return list(range(l))[-buffer_size:]


@pytest.mark.parametrize("bs,buf", [(64, 4096), (8, 32), (3, 9), (1, 4)])
def test_host_schedule_matches_the_reference_pool(bs, buf):
    from bnn_hip import bandit
    for l in list(range(1, 3 * buf + 2)) + [10000]:
        ref = _reference_pool(l, bs, buf)
        got = bandit.pool_entries(l, bs, buf)
        assert got.tolist() == ref, l                                             # same entries, same positions
        assert bandit.pool_size(l, bs, buf) == len(ref)
        # minibatches: range(0, len(idx_pool), batch_size) (base_bandit.py:87)
        assert bandit.n_batches(l - 1, bs, buf) == len(range(0, len(ref), bs))
        assert len(ref) % bs == 0


def test_beta_schedule():
    from bnn_hip import bandit
    for M in (1, 4, 64):
        b = [bandit.beta(j, M) for j in range(M)]
        assert b == [2 ** (M - (j + 1)) / (2 ** M - 1) for j in range(M)]     # bandits.py:44
        assert abs(sum(b) - 1.0) < 1e-12


def _params(**over):
    p = dict(buffer_size=32, batch_size=8, num_batches=4, lr=1e-3, hidden_units=16, mode="regression", mixture_prior=True,
             mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6], n_samples=2, epsilon=0.0)
    p.update(over)
    return p


def test_bandit_rejects_before_touching_a_device():
    import bnn_hip
    from bnn_hip import bandit, synth
    from bnn_hip.ops import BnnHipError
    x, y = synth.mushroom_like(64, 3)
    with pytest.raises(BnnHipError, match="local-reparameterisation"):
        bandit.BNNBandit("b", _params(), x, y, policy="thompson", local_reparam=True)
    with pytest.raises(BnnHipError, match="multiple of batch_size"):
        bandit.BNNBandit("b", _params(buffer_size=36), x, y)
    with pytest.raises(BnnHipError, match="buffer_size"):
        bandit.BNNBandit("b", _params(buffer_size=8192 + 8), x, y)
    with pytest.raises(BnnHipError, match="policy"):
        bandit.BNNBandit("b", _params(), x, y, policy="greedy")
    bnn_hip.shard_samples(True)
    try:
        with pytest.raises(BnnHipError, match="sharding"):
            bandit.BNNBandit("b", _params(), x, y, policy="mean")
    finally:
        bnn_hip.shard_samples(False)


def test_mushroom_like_and_table():
    from bnn_hip import bandit, synth
    x, y = synth.mushroom_like(1000, 7)
    assert x.shape == (1000, 117) and x.dtype == np.float32 and y.dtype == np.int64
    assert (x.sum(1) == 22).all() and set(np.unique(x)) == {0.0, 1.0}
    assert (y == 1).sum() == 500
    odor = x[:, 22:31].argmax(1)                                                  # the fifth attribute's 9 columns
    assert ((odor < 4) == (y == 1)).all()
    x2, y2 = synth.mushroom_like(1000, 7)
    assert np.array_equal(x, x2) and np.array_equal(y, y2)
    t = np.asarray(bandit.MUSHROOM.rewards)
    assert t.shape == (2, 2, 3) and bandit.MUSHROOM.oracle == (0.0, 5.0)
    assert tuple(t[1, 0, :2]) == (5, 5) and tuple(t[0, 0, :2]) == (5, -35) and t[0, 0, 2] == 0.5 and (t[:, 1, :2] == 0).all()
