"""bnn_hip.capture on CPU tensors (no GPU, no library): the uint32 word encoding, the optimiser's shared sample counter, the
optimiser snapshot around a warm-up step, the flat gradient bucket.  A plain torch optimiser with a hand-set `_dev` stands in
for FusedAdam / FusedSGD / FusedSGMCMC: the snapshot only knows their `_dev[gi]` layouts."""
import pytest
import torch

import bnn_hip
from bnn_hip import capture
from bnn_hip.runtime import state

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _restore():
    bnn_hip.manual_seed(2026)
    yield
    bnn_hip.manual_seed(2026)


# ---------------------------------------------------------------------------------------------------- the word encoding
@pytest.mark.parametrize("value", [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, (1 << 32) + 5])
def test_word32_round_trips_through_an_int32_tensor(value):
    w = capture.word32(value)
    assert -(1 << 31) <= w < (1 << 31)
    t = torch.zeros(1, dtype=torch.int32)
    t.fill_(w)
    assert int(t.item()) & 0xFFFFFFFF == value % (1 << 32)


# ---------------------------------------------------------------------------------------------------- the shared counter
def _sgd(n=2, lr=0.1):
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(3, 2 + i)) for i in range(n)]
    return torch.optim.SGD(params, lr=lr), params


def _device_value(sh):
    return int(sh["counter"].item()) & 0xFFFFFFFF


def test_two_users_of_one_optimiser_share_one_counter():
    bnn_hip.manual_seed(2026, 77)
    opt, _ = _sgd()
    a = capture.SampleCounter.of(opt, CPU)
    b = capture.SampleCounter.of(opt, CPU)
    assert a is b is opt._sample_words and a["counter"].dtype == torch.int32 and a["counter"].shape == (1,)
    assert a["base"] == 77 and a["mirror"] == 0 and state.counter == 77          # creating it draws nothing
    a.advance(3)
    assert b["mirror"] == 3
    other, _ = _sgd()
    assert capture.SampleCounter.of(other, CPU) is not a


def test_a_counter_on_another_device_is_replaced():
    opt, _ = _sgd()
    a = capture.SampleCounter.of(opt, CPU)
    a["counter"] = torch.zeros(1, dtype=torch.int32, device="meta")           # no second device here: a word that lives elsewhere
    state.counter = 11
    b = capture.SampleCounter.of(opt, CPU)
    assert b is not a and b is opt._sample_words and b["counter"].device == CPU and b["base"] == 11 and b["mirror"] == 0


def test_sync_fills_only_when_host_and_mirror_differ():
    bnn_hip.manual_seed(2026, 100)
    opt, _ = _sgd()
    sh = capture.SampleCounter.of(opt, CPU)
    v = sh["counter"]._version
    sh.sync()
    assert sh["counter"]._version == v and sh["mirror"] == 0                      # in step: nothing written
    state.counter = 105                                                     # an evaluation drew five indices
    sh.sync()
    assert sh["counter"]._version == v + 1 and sh["mirror"] == 5 == _device_value(sh)
    sh.sync()
    assert sh["counter"]._version == v + 1
    sh.set(9)
    assert sh["counter"]._version == v + 2 and sh["mirror"] == 9 == _device_value(sh)
    state.counter = 99                                                      # the host counter wrapped below the base
    sh.sync()
    assert sh["mirror"] == (1 << 32) - 1 == _device_value(sh)


def test_advance_moves_host_counter_and_mirror_together_and_wraps():
    bnn_hip.manual_seed(2026, (1 << 32) - 4)
    opt, _ = _sgd()
    sh = capture.SampleCounter.of(opt, CPU)
    sh.set((1 << 32) - 2)
    v = sh["counter"]._version
    state.counter = (sh["base"] + sh["mirror"]) & 0xFFFFFFFF
    sh.advance(5)                                                           # (the captured step moved the device word itself)
    assert sh["mirror"] == 3 and state.counter == (sh["base"] + 3) & 0xFFFFFFFF and sh["counter"]._version == v
    sh["counter"].fill_(capture.word32(3))
    v = sh["counter"]._version
    sh.sync()
    assert sh["counter"]._version == v                                        # still in step after the wrap


# ---------------------------------------------------------------------------------------------------- snapshot / restore
def _adam_with_history(lr=0.1):
    torch.manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(4))]
    opt = torch.optim.Adam(params, lr=lr)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    for p in params:                                                        # the fused optimisers keep a host int here
        opt.state[p]["step"] = 7
    return opt, params


def _adam_dev(step, lr):
    """FusedAdam's _dev[gi]: step int32[1], lr float32[1], last lr written, ticket int32[16]."""
    return [torch.tensor([step], dtype=torch.int32), torch.tensor([lr], dtype=torch.float32), lr, torch.zeros(16, dtype=torch.int32)]


def _warm_step(opt, params, dev_writes=()):
    """What a warm-up step does: moves the parameters, the optimiser state and the given device entries."""
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
            st = opt.state[p]
            if not st:
                st["step"] = 0
                st["exp_avg"], st["exp_avg_sq"] = torch.full_like(p, 3.0), torch.full_like(p, 4.0)
            else:
                st["exp_avg"].mul_(2.0).add_(1.0)
                st["exp_avg_sq"].add_(5.0)
                st["step"] = st["step"] + 1
    for d, i, v in dev_writes:
        d[i].fill_(v) if torch.is_tensor(d[i]) and not torch.is_tensor(v) else d.__setitem__(i, v)
    state.counter = (state.counter + 2) & 0xFFFFFFFF


def test_restore_puts_existing_state_back_in_place():
    opt, params = _adam_with_history()
    opt._dev = {0: _adam_dev(7, 0.1)}
    extra = [torch.arange(5.0), torch.ones(2)]
    before_p = [p.detach().clone() for p in params]
    before_m = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    ptrs = [(p.data_ptr(), opt.state[p]["exp_avg"].data_ptr(), opt.state[p]["exp_avg_sq"].data_ptr()) for p in params]
    dev_ptrs = [w.data_ptr() for w in opt._dev[0] if torch.is_tensor(w)]
    before_x = [t.clone() for t in extra]
    state.counter = 40
    restore = capture.snapshot(opt, extra=extra)
    d = opt._dev[0]
    _warm_step(opt, params, [(d, 0, 8), (d, 3, 1)])
    for t in extra:
        t.mul_(-3.0)
    restore()
    assert state.counter == 40
    for p, q, (m, v), ptr in zip(params, before_p, before_m, ptrs):
        st = opt.state[p]
        assert torch.equal(p.detach(), q) and torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v)
        assert st["step"] == 7 and (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) == ptr
    assert all(torch.equal(t, s) for t, s in zip(extra, before_x))
    assert int(d[0]) == 7 and float(d[1]) == pytest.approx(0.1) and d[2] == 0.1 and not d[3].any()
    assert [w.data_ptr() for w in d if torch.is_tensor(w)] == dev_ptrs


def test_state_the_warm_up_created_is_zeroed_and_its_step_word_starts_from_the_host_step():
    opt, params = _adam_with_history()
    fresh = torch.nn.Parameter(torch.randn(2, 2))                           # a parameter without state, in a group of its own
    opt.add_param_group(dict(params=[fresh]))
    opt._dev = {}
    restore = capture.snapshot(opt)
    _warm_step(opt, params + [fresh])
    opt._dev = {0: _adam_dev(1, 0.1), 1: _adam_dev(1, 0.1)}                  # created by the warm-up, counted one step
    restore()
    st = opt.state[fresh]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and st["step"] == 0
    assert int(opt._dev[0][0]) == 7                                         # the host-side step of the group's parameters
    assert int(opt._dev[1][0]) == 0                                         # no history: a fresh optimiser's


def test_sgd_layout_is_restored_and_a_created_one_is_left_alone():
    opt, params = _sgd(lr=0.1)
    opt._dev = {0: [torch.tensor([0.1]), 0.1]}                              # FusedSGD: lr float32[1], last lr written
    restore = capture.snapshot(opt)
    d = opt._dev[0]
    ptr = d[0].data_ptr()
    d[0].fill_(0.3)
    d[1] = 0.3
    restore()
    assert float(d[0]) == pytest.approx(0.1) and d[1] == 0.1 and d[0].data_ptr() == ptr
    opt2, _ = _sgd(lr=0.2)
    opt2._dev = {}
    restore = capture.snapshot(opt2)
    opt2._dev = {0: [torch.tensor([0.2]), 0.2]}                             # created by the warm-up: there is no step word
    restore()
    assert float(opt2._dev[0][0]) == pytest.approx(0.2) and opt2._dev[0][1] == 0.2


def test_sgmcmc_layout_with_a_trailing_bank_is_restored():
    opt, params = _sgd()
    bank = torch.arange(4096.0).reshape(4, 1024)
    table = torch.tensor([[0.05, 0.0, 0.3, 1.0]])
    opt._dev = {0: [torch.tensor([12], dtype=torch.int32), torch.tensor([3], dtype=torch.int32),
                    torch.zeros(16, dtype=torch.int32), table, 0.1, bank]}   # step, collected, ticket, table, lr, the bank's ring
    want = [w.clone() if torch.is_tensor(w) else w for w in opt._dev[0]]
    ptrs = [w.data_ptr() for w in opt._dev[0] if torch.is_tensor(w)]
    restore = capture.snapshot(opt)
    d = opt._dev[0]
    d[0].add_(1)
    d[1].add_(1)
    d[3].mul_(0.5)
    d[4] = 0.05
    bank[1].fill_(-1.0)                                                     # the warm-up filed its weights over a member
    restore()
    for got, w in zip(d, want):
        assert torch.equal(got, w) if torch.is_tensor(w) else got == w
    assert [w.data_ptr() for w in d if torch.is_tensor(w)] == ptrs and d[5] is bank


@pytest.mark.parametrize("layout", ["adam", "sgd"])
def test_a_warm_up_that_wrote_a_new_learning_rate_leaves_word_and_last_written_a_pair(layout):
    """A step object built after param_groups[0]['lr'] changed: the warm-up's sync_lr() writes the new rate into the word and
    into 'last written'.  Restoring only the word would leave 'last written' at the new rate: every later sync_lr() would
    skip the write and the captured graph would train on the old rate."""
    opt, params = _adam_with_history(lr=0.1) if layout == "adam" else _sgd(lr=0.1)
    word, last = (1, 2) if layout == "adam" else (0, 1)
    opt._dev = {0: _adam_dev(7, 0.1) if layout == "adam" else [torch.tensor([0.1]), 0.1]}
    d = opt._dev[0]
    opt.param_groups[0]["lr"] = 0.05
    restore = capture.snapshot(opt)
    _warm_step(opt, params, [(d, word, 0.05), (d, last, 0.05)])              # the warm-up's sync_lr()
    restore()
    assert float(d[word]) == pytest.approx(0.1) and d[last] == 0.1
    assert d[last] != opt.param_groups[0]["lr"]                             # so the next sync_lr() writes 0.05


# ---------------------------------------------------------------------------------------------------- the bucket
@pytest.mark.parametrize("never_empty", [False, True])
def test_grad_bucket_layout(never_empty):
    params = [torch.zeros(n) for n in (1, 63, 64, 65, 0)]
    bucket, offs = capture.grad_bucket(params, CPU, never_empty=never_empty)
    assert offs == [0, 64, 128, 192, 320]
    assert bucket.numel() == (384 if never_empty else 320) and bucket.dtype == torch.float32 and not bucket.any()
    views = [bucket[o:o + p.numel()] for o, p in zip(offs, params)]
    for i, (v, o) in enumerate(zip(views, offs)):
        v.fill_(i + 1.0)
        assert o % 64 == 0 and (v.numel() == 0 or v.data_ptr() == bucket.data_ptr() + 4 * o)
    assert bucket[0] == 1 and bucket[64 + 62] == 2 and bucket[64 + 63] == 0 and bucket[128 + 63] == 3 and bucket[192 + 64] == 4
    assert float(bucket.sum()) == 1 + 2 * 63 + 3 * 64 + 4 * 65
