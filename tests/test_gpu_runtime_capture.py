"""What the whole-step runners of xequinet_amd/runtime.py share, where no other test reaches it: the "weights moved, capture again" step on
GraphedLanes and GraphedStepPBC (a bumped pack epoch: tests/test_gpu_fullsize.py moves the weights under a GraphedStep only), and the
edge counters of all four open-boundary runners around a capture INSIDE the counted window (its warm-up runs are not steps) and around
zero_edge_total().

Sizes: four molecules of 3, 4, 5 and 6 atoms (data/synthetic.synth_molecule, seeded) at three scales -- 68, 60 and 38 edges counted on the
host: at the first every pair is inside the cutoff -- as two lanes / two chunks, both in flight; one water molecule in a 3.1 A box (images
on every axis).  Model: hessian_cases.model_case("well")."""
import copy

import numpy as np
import pytest
import torch

from tests import hessian_cases as hc
from xequinet_amd.data import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALES = (1.0, 2.0, 3.0)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.fixture(scope="module")
def model():
    return copy.deepcopy(hc.model_case("well")[0]).to(device=DEV, dtype=torch.float32).eval().requires_grad_(False)


@pytest.fixture(scope="module")
def molecules(model):
    """(draws, ptr_host, capacity, true edge counts): the same four molecules at the three SCALES as (pos, z, ptr, batch) on the device, and
    each draw's edge count from a lone GraphedStep's own output (not from its running counter)."""
    from xequinet_amd import runtime

    rng = np.random.default_rng(11)
    mols = [syn.synth_molecule(rng, n) for n in (3, 4, 5, 6)]
    pos, z = np.concatenate([p for p, _ in mols]), np.concatenate([q for _, q in mols])
    ptr = np.array([0, 3, 7, 12, 18], dtype=np.int64)
    batch = np.repeat(np.arange(4), np.diff(ptr))
    draws = [(_t(pos * s, torch.float32), _t(z), _t(ptr), _t(batch)) for s in SCALES]
    cap = (len(pos), 4, runtime.pair_capacity(ptr))
    lone = runtime.GraphedStep(model, cap)
    counts = [int(lone(*d[:3], batch=d[3])["n_edges"].item()) for d in draws]
    assert counts[0] == cap[2] and len(set(counts)) == 3, counts      # every pair at the first scale, fewer and different at the others
    return draws, ptr, cap, counts


def _same_after_the_epoch_moved(runner, call, first, other):
    """``call(inputs) -> results``: one capture on the first call, none on a call with other positions, exactly one more behind a bumped
    pack epoch -- and, the weights being what they were, the very bits of the first call."""
    from xequinet_amd import lib

    before = {k: v.clone() for k, v in call(first).items()}
    assert runner.captures == 1
    call(other)
    assert runner.captures == 1
    lib.bump_pack_epoch()
    after = {k: v.clone() for k, v in call(first).items()}
    assert runner.captures == 2
    assert set(after) == set(before) and {"energy", "forces"} <= set(after)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    call(other)
    assert runner.captures == 2


def test_lanes_capture_again_behind_a_bumped_pack_epoch(model, molecules):
    from xequinet_amd import runtime

    draws, ptr, cap, _ = molecules
    lanes = runtime.GraphedLanes(model, cap, lanes=2)
    _same_after_the_epoch_moved(lanes, lambda d: lanes(*d, ptr), draws[0], draws[1])
    assert not lanes.overflowed()


def test_periodic_step_captures_again_behind_a_bumped_pack_epoch(model):
    from xequinet_amd import runtime

    pos, z, _, cell = syn.synth_water_box(1, seed=3)
    assert len(pos) == 3
    cell_d, pbc = _t(np.asarray(cell).reshape(3, 3), torch.float32), [True, True, True]
    first, other = _t(pos, torch.float32), _t(pos + np.array([[0.05, 0.0, 0.0], [0.0, -0.05, 0.0], [0.0, 0.0, 0.05]]), torch.float32)
    step = runtime.GraphedStepPBC(model, 3, 4096)         # (room for every image pair: a list that outgrew it would capture again by itself)
    _same_after_the_epoch_moved(step, lambda p: step(p, _t(z), cell_d, pbc), first, other)
    assert not step.overflowed() and int(step.outputs["n_edges"].item()) > 6    # images were seen


def _runners(name, model, cap, ptr):
    """-> (object, call(draw), zero())"""
    from xequinet_amd import runtime

    if name == "GraphedStep":
        r = runtime.GraphedStep(model, cap)
        return r, (lambda d: r(*d[:3], batch=d[3])), (lambda: r.edge_total.zero_())
    if name == "GraphedLanes":
        r = runtime.GraphedLanes(model, cap, lanes=2)
        return r, (lambda d: r(*d, ptr)), r.zero_edge_total
    if name == "GraphedStepsInFlight":
        r = runtime.GraphedStepsInFlight(model, cap, depth=2)
        return r, (lambda d: r(*d)), r.zero_edge_total
    r = runtime.GraphedChunks(model, ptr, max_edges=40, depth=2)
    assert r.n_chunks >= 2 and r.depth == 2
    return r, (lambda d: r(*d)), r.zero_edge_total


@pytest.mark.parametrize("name", ["GraphedStep", "GraphedLanes", "GraphedStepsInFlight", "GraphedChunks"])
def test_edge_total_counts_the_steps_of_the_window_only(name, model, molecules):
    """zero_edge_total(), three calls, the first of which captures: the counter holds the three true edge counts, not the warm-up runs'.
    Then the same window again behind a bumped pack epoch: the counter starts from zero again and the second capture's warm-up runs
    are not counted either."""
    from xequinet_amd import lib

    draws, ptr, cap, counts = molecules
    runner, call, zero = _runners(name, model, cap, ptr)
    for window in range(2):
        zero()
        for d in draws:
            call(d)
        assert int(runner.edge_total) == sum(counts), (name, window)
        lib.bump_pack_epoch()
    assert not runner.overflowed()
