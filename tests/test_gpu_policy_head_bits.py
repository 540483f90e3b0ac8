"""The policy-head kernels on the device against the bits recorded from the commit before their expressions and wave
primitives were stated once (tests/golden/policy_head_device_bits.npz, made by tests/golden/make_policy_head_bits.py): the
calls of tests/policy_head_cases.py replayed and compared bit for bit.  The device's expf / logf belong to the toolchain, so a
mismatch quotes the toolchain the fixture was recorded with and the one that built the running library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_head_cases  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    return policy_head_cases


@pytest.fixture(scope="module")
def recorded():
    return load_golden(policy_head_cases.FIXTURE)


def compare(pc, recorded, got):
    for name, value in got.items():
        assert pc.same_bits(value, recorded[name]), \
            "%s differs from the recorded bits (recorded with: %s; running: %s)" % (name, recorded["toolchain"], pc.toolchain())


@pytest.mark.parametrize("E,M", policy_head_cases.EVAL_SHAPES)
def test_gpu_evaluate_and_a2c_loss_give_the_recorded_bits(pc, recorded, E, M):
    got, bwd = pc.eval_case(E, M)
    assert len(got) == 6
    compare(pc, recorded, got)
    compare(pc, recorded, {"a2c_grad_logits_E%d_M%d" % (E, M): bwd})      # the backward kernel under the normative weights


@pytest.mark.parametrize("M", policy_head_cases.ACT_WAVE_MS + policy_head_cases.ACT_LANES_MS)
def test_gpu_masked_act_gives_the_recorded_actions_and_log_probabilities(pc, recorded, M):
    got = pc.act_case(M)
    assert len(got) == 8
    compare(pc, recorded, got)


@pytest.mark.parametrize("M", policy_head_cases.SAMPLE_MS)
def test_gpu_sample_feasible_gives_the_recorded_actions(pc, recorded, M):
    got = pc.sample_case(M)
    assert len(got) == 2 and all(v.min() >= 0 for v in got.values())
    compare(pc, recorded, got)


def test_the_fixture_holds_nothing_that_is_not_replayed(pc, recorded):
    names = set()
    for E, M in pc.EVAL_SHAPES:
        names |= {"%s_E%d_M%d" % (k, E, M) for k in ("evaluate_logp", "evaluate_entropy", "evaluate_bad", "a2c_rows", "a2c_terms", "a2c_grad_logits")}
    for M in pc.ACT_WAVE_MS + pc.ACT_LANES_MS:
        names |= {"act_%s_M%d_base%d_%s" % (k, M, b, d) for k in ("action", "logp") for b in (0, 1) for d in ("mode", "sample")}
    names |= {"sample_M%d_base%d" % (M, b) for M in pc.SAMPLE_MS for b in (0, 1)}
    assert set(recorded) == names | {"toolchain"}
