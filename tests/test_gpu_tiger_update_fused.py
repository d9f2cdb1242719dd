"""reject_tiger_once_kernel on its clean path (no word set outside the action's four) stores a record of the new filter from the thread
whose attempt was accepted, inside the attempt loop: `j < N` guards a store to global memory there, and a record stored at j >= N would
land in the next slot's buffer.  So: filters that are no multiple of the 512 attempts of a round (the last round always overshoots N), at
130 slots, every slot's final filter compared -- with the generic reject_kernel on dense records (FBA_DENSE_PARTICLES=1), with the oracle,
and with the path that lists its accepted attempts and gathers them behind the loop (FBA_TIGER_GATHER=1), bit for bit as in
tests/test_gpu_tiger_update_once.py, whose comparisons these are."""
import pytest

from test_gpu_tiger_update_once import (_assert_equals_oracle, _assert_every_kind_of_slot_occurred, _assert_same_contexts, _engine, _run)

pytestmark = pytest.mark.gpu

SLOTS = 130      # two whole waves of slots and three more


def _seed(particles):
    return 9100 + particles + SLOTS      # the rule of test_gpu_tiger_update_once.py: 12815, 13069, 13325 and (continuous tiger) 12815, 13325


@pytest.mark.parametrize("particles", [3585, 3839, 4095])
def test_clean_path_at_ragged_sizes_equals_dense_records_and_the_oracle(particles, monkeypatch):
    """episodic tiger: every update is a `listen` on records that hold nothing but the listen words, 4 699-16 326 attempts each"""
    domain, seed = "episodic-tiger", _seed(particles)
    packed = _engine(domain, "rejection_sampling", particles, SLOTS, seed, monkeypatch)
    dense = _engine(domain, "rejection_sampling", particles, SLOTS, seed, monkeypatch, FBA_DENSE_PARTICLES="1")
    assert packed.particle_bytes == 64 and dense.particle_bytes == 128
    rp, rd = _run(packed), _run(dense)
    _assert_same_contexts(packed, dense, rp, rd, SLOTS)
    _assert_every_kind_of_slot_occurred(rp[0], domain, SLOTS)
    _assert_equals_oracle(domain, "rejection_sampling", particles, SLOTS, seed, rp)


@pytest.mark.parametrize("particles", [3585, 3839, 4095])
def test_storing_in_the_loop_equals_listing_and_gathering(particles, monkeypatch):
    domain, seed = "episodic-tiger", _seed(particles)
    stored = _engine(domain, "rejection_sampling", particles, SLOTS, seed, monkeypatch)
    gathered = _engine(domain, "rejection_sampling", particles, SLOTS, seed, monkeypatch, FBA_TIGER_GATHER="1")
    rs, rg = _run(stored), _run(gathered)
    _assert_same_contexts(stored, gathered, rs, rg, SLOTS)
    _assert_every_kind_of_slot_occurred(rs[0], domain, SLOTS)


@pytest.mark.parametrize("particles", [3585, 4095])
def test_both_paths_in_one_run_equal_dense_records_and_the_oracle(particles, monkeypatch):
    """continuous tiger: a run stores in the loop before its first `open` and lists and gathers after it (the helper asserts both occurred)"""
    domain, seed = "continuous-tiger", _seed(particles)
    packed = _engine(domain, "rejection_sampling", particles, SLOTS, seed, monkeypatch)
    dense = _engine(domain, "rejection_sampling", particles, SLOTS, seed, monkeypatch, FBA_DENSE_PARTICLES="1")
    rp, rd = _run(packed), _run(dense)
    _assert_same_contexts(packed, dense, rp, rd, SLOTS)
    _assert_every_kind_of_slot_occurred(rp[0], domain, SLOTS)
    _assert_equals_oracle(domain, "rejection_sampling", particles, SLOTS, seed, rp)
