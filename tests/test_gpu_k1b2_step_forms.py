"""The step bodies of the pair block GEMM K1b2 (csrc/bbb_linear.hip): a wave picks the body of its k-step once, ahead of the loop
-- Gaussian prior without epsilon dump x {no statistics, statistics, statistics + sum of log sigma}, the generic body for a mixture
prior or an epsilon dump, masked steps at the edges, nothing but staging for a phantom wave -- and the waves of one block run
different bodies across the same barriers.  Whatever runs, the bits are the same: every comparison here is BIT equality, between
launches of the built library that differ in the body they select, and against sha256 digests recorded with the library of the commit
before the bodies existed (tests/golden/k1b2_step_forms_parent.json; tools/k1b2_step_forms.py is the case list, the launcher and
the recorder).  Every launch is forced to the block form with a hoisted sigma and asserts `waves == 8` from its plan."""
import json
import os
import sys

import pytest
import torch

import bnn_hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import k1b2_step_forms as SF          # noqa: E402

pytestmark = pytest.mark.gpu

CASES = SF.case_names()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def record():
    with open(SF.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _bf16_math():
    bnn_hip.set_math("bf16")
    yield
    bnn_hip.set_math("bf16")


@pytest.fixture(scope="module")
def full(dev):
    """Per case: the launch with statistics and epsilon dump (computed once, never modified)."""
    res = {name: SF.launch(*SF.parse(name), dev) for name in CASES}
    torch.cuda.synchronize()
    return res


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).reshape(-1)


def test_the_record_covers_the_case_list(record):
    assert sorted(record) == sorted(CASES)
    assert all(sorted(v) == sorted(SF.TENSORS) for v in record.values())


@pytest.mark.parametrize("name", CASES)
def test_bits_equal_the_parent_commits(full, record, name):
    """y, the per-sample scalars and the dumped epsilon: every bit as the parent commit's build wrote it."""
    got = {k: SF.digest(full[name][k]) for k in SF.TENSORS}
    assert got == record[name], (name, [k for k in got if got[k] != record[name].get(k)])


@pytest.mark.parametrize("name", CASES)
def test_without_the_epsilon_dump(dev, full, name):
    """dump_eps=False (the waves of the samples' first batch block leave the generic body): y, log_prior, log_q bit-equal."""
    out = SF.launch(*SF.parse(name), dev, dump_eps=False)
    assert out["eps_w"] is None and out["eps_b"] is None
    for k in ("y", "log_prior", "log_q"):
        assert torch.equal(bits(out[k]), bits(full[name][k])), k


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dump_eps", [False, True])
def test_without_statistics(dev, full, name, dump_eps):
    """want_stats=False (every wave in the body without statistics, or the generic one with the dump): y bit-equal."""
    out = SF.launch(*SF.parse(name), dev, want_stats=False, dump_eps=dump_eps)
    assert torch.equal(bits(out["y"]), bits(full[name]["y"]))
    if dump_eps:
        for k in ("eps_w", "eps_b"):
            assert torch.equal(bits(out[k]), bits(full[name][k])), k


@pytest.mark.parametrize("name", CASES)
def test_equals_the_register_form(dev, full, name):
    """K1b (no hoisted sigma: parameters in registers, row-major operands) gives the same y."""
    shape, layout, prior = SF.parse(name)
    out = SF.launch(shape, "rows", prior, dev, hoisted=False, dump_eps=False)
    assert torch.equal(bits(out["y"]), bits(full[name]["y"]))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dump_eps", [False, True])
def test_two_launches_give_identical_bits(dev, full, name, dump_eps):
    a = SF.launch(*SF.parse(name), dev, dump_eps=dump_eps)
    b = SF.launch(*SF.parse(name), dev, dump_eps=dump_eps)
    for k in SF.TENSORS:
        if a[k] is None:
            assert not dump_eps and k in ("eps_w", "eps_b")
            continue
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert torch.equal(bits(a[k]), bits(full[name][k])), k
