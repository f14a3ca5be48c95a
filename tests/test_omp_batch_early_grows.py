"""A batch compress call of different shapes whose single-call item is LARGER than all of its batched items together (szhip_compress_omp_batch_shapes).

The call sizes the context's work arrays for the items of the shared launches; the item that goes through the single call from inside it (boxes of no multiple of
8 points) runs before the shared sweeps and, on a fresh context, asks for more than that: the context allocates the arrays anew, and the shared launches must use them
where they lie from then on (sz_amd/csrc/szhip_ompbatch.inc, the context buffers of ompb_enc).  tests/test_omp_batch_shapes.py does not reach this: its single-call
items are smaller than the batched ones.  The bar is that file's, with no tolerance: every item's stream is byte for byte the oracle's of the array alone, and the decode
of the oracle's streams gives the oracle's arrays bit for bit.

The items: b8, 16^3 in 8^3 boxes (4096 values, batched), and p5670, (36, 30, 42) / 8 in boxes of 18 x 15 x 21 = 5670 points (45 360 values, the single call): the
smallest pair of that file's kind in which the single call's item outgrows eleven batched 16^3 arrays.  Every test has a context of its own, so nothing is allocated
before the call.  Both orders of the two, with the interval optimiser and with fixed intervals, one test each; on the CPU shim and, under -m gpu, through the built library."""
import pytest

import test_omp_batch_shapes as shapes
from test_omp_batch import FIXED_INTERVALS, hip_ctx, shim_ctx  # noqa: F401  (the two fixtures)

shapes.KINDS.setdefault("p5670", ((36, 30, 42), 8))      # (a kind of this file alone: no batch of test_omp_batch_shapes.py names it)
ORDERS = (["b8/a", "p5670/a"], ["p5670/a", "b8/a", "b8/16"])
CASES = [(k, iv) for k in range(len(ORDERS)) for iv in (0, FIXED_INTERVALS)]
IDS = [f"order{k}-intervals{iv}" for k, iv in CASES]


def _early_item_grows(ctx, oracle, device, k, iv):
    batch = ORDERS[k]
    items, _, _ = shapes.compress(ctx, oracle, batch, device, iv)
    assert [it.batched for it in items] == [0 if n.startswith("p") else 1 for n in batch]
    shapes.decode(ctx, oracle, batch, device, iv=iv)


@pytest.mark.parametrize("k,iv", CASES, ids=IDS)
def test_early_item_grows_on_cpu_shim(oracle, shim_ctx, k, iv):
    _early_item_grows(shim_ctx, oracle, False, k, iv)


@pytest.mark.gpu
@pytest.mark.parametrize("k,iv", CASES, ids=IDS)
def test_hip_early_item_grows(oracle, hip_ctx, k, iv):
    _early_item_grows(hip_ctx, oracle, True, k, iv)
