"""`data.val_batches`: the index plan of a validation pass (no GPU needed)."""
import numpy as np
import pytest

from lunaris_orion_amd.data import val_batches


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("batch", [4, 64])
@pytest.mark.parametrize("n_val", [0, 1, 7, 64, 65])
def test_val_batches_cover_every_index_once_with_equal_batch_counts(n_val, batch, world):
    val_idx = np.random.default_rng(n_val * 100 + batch + world).permutation(1000)[:n_val] + 5000
    plans = [list(val_batches(val_idx, batch, rank, world)) for rank in range(world)]
    assert len({len(p) for p in plans}) == 1                                  # every rank the same number of batches
    if n_val == 0:
        assert plans[0] == []                                                 # nothing to validate: the CLI logs that it skips
        return
    assert len(plans[0]) == -(-(-(-n_val // world)) // batch)                 # ceil(ceil(n_val / world) / batch): no batch to spare
    seen = []
    for plan in plans:
        for idx, n_valid in plan:
            assert idx.shape == (batch,) and idx.dtype == np.int64 and 0 <= n_valid <= batch
            seen.extend(idx[:n_valid].tolist())
            if 0 < n_valid < batch:
                assert set(idx[n_valid:].tolist()) <= set(idx[:n_valid].tolist())   # padding repeats an index of the same batch
            elif n_valid == 0:
                assert set(idx.tolist()) <= set(val_idx.tolist())             # a spent rank still feeds the engine real sprites
    assert sorted(seen) == sorted(val_idx.tolist())                           # every held-out index exactly once across ranks
    assert sum(n for plan in plans for _, n in plan) == n_val
