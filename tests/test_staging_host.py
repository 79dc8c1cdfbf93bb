"""CPU: the two device-free pieces of torchdet3d/dataloaders/staging.py -- `pack`, the layout of the one pinned upload, and
`StagedLoader._batches`, the prefetch loop, at `prefetch = 0` with a `finish` that touches no device."""
import numpy as np
import pytest

from torchdet3d.dataloaders.staging import StagedLoader, pack


def test_pack_lays_the_parts_out_aligned_in_order_and_apart():
    sizes = (0, 1, 15, 16, 17, 240)
    rng = np.random.default_rng(0)
    parts = [rng.integers(0, 256, n).astype(np.uint8) for n in sizes]
    offs, total = pack(parts, 16)
    padded = [-(-n // 16) * 16 for n in sizes]
    assert len(offs) == len(parts) and all(o % 16 == 0 for o in offs)
    assert all(offs[k] + sizes[k] <= offs[k + 1] for k in range(len(offs) - 1)), 'out of order or overlapping'
    assert total == offs[-1] + padded[-1] == sum(padded)
    buf = np.full(total, 0xEE, np.uint8)
    for p, o in zip(parts, offs):
        buf[o:o + p.size] = p
    for p, o in zip(parts, offs):
        assert np.array_equal(buf[o:o + p.size], p)
    assert pack([], 16) == ([], 0)


@pytest.mark.parametrize('n', [0, 1, 5])
def test_the_prefetch_loop_finishes_every_item_once_in_order_and_one_ahead_at_most(n):
    loader = StagedLoader(prefetch=0, min_staging=1)
    finished, taken, got = [], [], []

    def source():
        for i in range(n):
            taken.append(i)
            yield ('item', i)

    def finish(item, key_tail):
        assert key_tail == (len(finished),)                 # the batch number keys the draws
        assert len(got) == len(finished), 'finish ran more than one item ahead of the consumer'
        finished.append(item)
        return (item, key_tail), None                       # (tensors, no ready event: nothing to wait for)
    for out in loader._batches(source(), finish):
        got.append(out)
        assert len(finished) == len(taken) == len(got)
    assert finished == [('item', i) for i in range(n)]
    assert got == [(('item', i), (i,)) for i in range(n)]
