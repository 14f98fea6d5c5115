"""The random walk over the device API on chunk images (lifecycle_walk.py)
against the kernels: one DevWriter and one Crc32DevPlan per walk, every call
over a slice of the same tensors, the composed models in lock step and the
ledger beside them.  test_lifecycle_walk_model.py runs the same walks -- the
same ops, seed by seed -- on the models alone.

sync_every = 1: after every op the statuses and every other output array
(pre-filled, so an entry the call forgot shows) and ALL the call may touch --
the whole buffer, offsets, capacities, crc_cur, the transaction state, the
arena words, the list and its count -- are compared with the Store.
sync_every = 8: eight ops are queued on the stream with nothing read back in
between; then the eight sets of outputs and the state are compared.

Every 10 ops and at the end verify_batch_dev must accept every finished chunk
and read_packed_batch_dev of list + live must give the ledger's contents.  A
failure names the profile, the seed, the op's index and its description; the
walk is a function of (profile, seed) alone, so a rerun reproduces it."""
import pytest

import lifecycle_walk as lw

pytestmark = pytest.mark.gpu

SEEDS = (1, 4, 7)                             # 4: a walk without CIO_CHECKSUM


@pytest.mark.parametrize("sync_every", [1, 8])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", sorted(lw.PROFILES))
def test_walk_on_the_device(cuda, profile, seed, sync_every):
    lw.walk(profile, seed, cuda=cuda, sync_every=sync_every)
