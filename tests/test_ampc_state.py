"""The AMPC shard driven through interleaved calls against one model (tests/ampc_model.py): tables, graphs and filters stay alive over a
whole sequence, as they do in run_harmonic_job, run_shortest_paths_job and run_approx_harmonic_job, and every public call of
stract_amd/ampc.py is made on them in a drawn order.  After every operation the call's own answer is compared exactly (actions, counts,
found flags, returned rows; floats by bit pattern), after every eighth and after every refused call the whole content of every live table
and filter.  One sequence per seed; the seed list is chosen from the model alone, and the first test holds it to the conditions (a) .. (m)
of DESIGN.md section 35 without a device."""
import pytest

from tests import ampc_model as model

SEEDS = [101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117, 118, 119, 120, 122, 123]


def test_the_seed_list_reaches_the_state_edges():
    """(a) .. (m) over the list, and both caps for every sequence: fewer than 5 % of the drawn operations dropped, fewer than 15 % refusals.
    The model alone: no library is loaded."""
    worlds = [model.run(seed) for seed in SEEDS]
    total = model.totals(worlds)
    print({k: total[k] for k in model.NEED})
    assert not model.unmet(worlds)
    assert max(w.counts["largest_table"] for w in worlds) > 1024
    assert sum(w.counts["largest_table"] > 512 for w in worlds) >= len(SEEDS) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_interleaved_calls_against_the_model(seed):
    from stract_amd import ampc
    assert ampc.wave_group_length() == model.WAVE_GROUP
    handles = model.Handles()
    try:
        model.run(seed, handles)
    finally:
        handles.close()
