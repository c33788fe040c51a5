"""A short run of the output-stage fuzzer (tools/fuzz_gpu_output.py) under -m gpu: the rounds of tests/output_fuzz_plan.py — windows x
filters x RGB output x tensor formats with flips x placements x warps x JPGPU_RS_ROLL — through Batch (two decodes per round on a
poisoned caller-owned arena, the knob-1 twin of every forced round) and, every fourth round, through one kept Pipeline; bit for bit
against the reference chain of the feature tests.  tests/test_output_fuzz_plan.py shows on the CPU which branches these very seeds and
round counts reach.

Rounds: the reference chain (oracle decode, rgb_ref, filter_ref, warp_ref, tensor_ref) of one seed's 26 rounds — two turns of the
thirteen templates, about 250 comparisons — took 3.0 s (seed 2026) and 2.8 s (seed 2027) on the development machine's CPU, 39 rounds
4.2 s and 5.6 s; the device side is a few dozen small launches per round.  26 rounds already reach every class at least three times
over the two seeds, so 26 it is: a few seconds per test function."""
import ast
import importlib.util
import os

import pytest

import output_fuzz_plan as OP

pytestmark = pytest.mark.gpu

ROUNDS = 26
SEEDS = [2026, 2027]


def _fuzzer():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_gpu_output.py")
    spec = importlib.util.spec_from_file_location("fuzz_gpu_output", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed", SEEDS)
def test_output_stage_fuzz_bit_exact(seed):
    bad, total, paths = _fuzzer().run(seed, ROUNDS, verbose=True)
    assert bad == 0, (bad, total, paths)
    assert total == OP.image_count(OP.plan(seed, ROUNDS)), (total, paths)  # (nothing left out)
    assert any("+roll" in p for p in paths) and any("+warp" in p for p in paths), paths
    assert any("+roll+warp" in p for p in paths) and any(p.startswith("pipeline ") for p in paths), paths


def test_replaying_a_round_alone_gives_its_comparisons():
    """`--replay`: the dict a mismatch prints, as a Python literal, runs that round alone."""
    rd = OP.plan(SEEDS[0], 8)[7]  # (a placed and warped round with a pipeline leg)
    assert rd["pipeline"] is not None and rd["warp"] is not None
    bad, total, _paths = _fuzzer().run(0, 1, verbose=True, replay=ast.literal_eval(repr(rd)))
    assert bad == 0 and total == OP.image_count([rd])
