"""Host-side tests of the sub-batch split a minibatch wider than one update pass runs as (ddpg.sub_batch_sizes, Agent.sub_batches):
the sizes, and the refusal of BATCH_SIZE > 1024 before any device work (a ninth sub-batch would sample with the next update's tick)."""
import importlib

import pytest

import util as U


def _d():
    U.pkg()
    return importlib.import_module(U.PKG_NAME + ".ddpg")


@pytest.mark.parametrize("batch,sizes", [(1, [1]), (128, [128]), (129, [65, 64]), (150, [75, 75]), (257, [86, 86, 85]),
                                         (1023, [128] * 7 + [127]), (1024, [128] * 8)])
def test_sub_batch_sizes_are_near_equal_and_at_most_eight(batch, sizes):
    D = _d()
    got = D.sub_batch_sizes(batch, D.Agent.MAX_PASS_BATCH)
    assert got == sizes and sum(got) == batch and len(got) <= D.MAX_SUB_BATCHES
    assert max(got) - min(got) <= 1 and got == sorted(got, reverse=True)


@pytest.mark.parametrize("batch", [1025, 2048, 0, -3])
def test_sub_batch_sizes_refuse_batches_outside_1_to_1024_naming_the_limit_and_reason(batch):
    D = _d()
    with pytest.raises(ValueError, match=r"1\.\.1024.*next update"):
        D.sub_batch_sizes(batch, D.Agent.MAX_PASS_BATCH)


def test_agent_sub_batches_refuses_before_any_device_work():
    """Agent.sub_batches (what replay() calls first for BATCH_SIZE > 128) raises before it allocates: an object with nothing but the
    batch and the pass width is enough to reach the refusal."""
    D = _d()

    class Bare:
        MAX_PASS_BATCH = D.Agent.MAX_PASS_BATCH
        batch = 1025

    with pytest.raises(ValueError, match="1024"):
        D.Agent.sub_batches(Bare())
