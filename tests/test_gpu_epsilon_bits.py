"""Everything that draws epsilon, bit for bit against the record in tests/golden/k1b2_parent_digests.json.

The record holds sha256 digests of the raw output bytes of a fixed list of launches (tools/epsilon_bits.py: the list, and
the recorder that wrote the file with the library of the commit BEFORE the generator's three-input xors, the packed
Box-Muller arithmetic and K1b2's phantom-wave / per-wave mask / prologue / epilogue changes).  Integer logic and
correctly rounded fp32 operations in a different instruction form give the same bits, so there is no tolerance: the
materialised epsilon stream, the block form K1b2 (bf16 and split-bf16 math, ReLU on and off, bf16 and fp32 outputs; y, the
dumped epsilon, log prior, log q) at shapes with phantom waves, a half-real tile, an idle pair slot, a partial k-step and
short batch blocks and at the benchmark's two hidden layers, the tile form K1a and the sampler K1s (which share the
generator's header), and one captured stacked evaluation (sums, per-pair outputs, logits)."""
import json
import os
import sys

import pytest
import torch

import bnn_hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import epsilon_bits as EB          # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def record():
    with open(EB.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def test_the_record_covers_the_case_list(record):
    assert sorted(record) == sorted(EB.case_names())


@pytest.mark.parametrize("name", EB.case_names())
def test_bits_equal_the_parent_commits(dev, record, name):
    got = EB.run_case(name, dev)
    assert got == record[name], (name, [k for k in got if got[k] != record[name].get(k)])
