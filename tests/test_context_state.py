"""One context driven through interleaved calls of every call family against one model (tests/context_model.py):
hb_run / hb_begin / hb_step / hb_finish, the ten operators with arguments that change from call to call, loads of other graphs in the
middle, hb_release_cached_memory and the refusals of the sibling suites, in a drawn order on a context that stays open.  After every
call its own answer is compared as the operator's suite compares it; after every refusal, after every sixth operation and at the end
every reader of every operator is called, one C entry point at a time: a live result reads byte for byte what the device returned when
it was made, a result that is gone is refused by each of its readers.  One sequence per seed; the seed list is chosen from the model alone, and the first test holds it to the conditions
(a) .. (k) of section 36 without a device."""
import pytest

from tests import context_model as model

SEEDS = [601, 602, 603, 604, 605, 606, 607, 608, 609, 610, 611, 612, 613]  # the first from 601 on; each keeps both caps


def test_the_seed_list_reaches_the_state_edges():
    """(a) .. (k) over the list, and both caps for every sequence: fewer than 5 % of the drawn operations dropped, fewer than 15 % refusals.
    The model alone: no library is loaded."""
    from stract_amd import _lib
    before = (_lib._lib, _lib._lib_exp)
    worlds = [model.run(seed) for seed in SEEDS]
    total = model.totals(worlds)
    print({k: total[k] for k in model.NEED})
    assert not model.unmet(worlds)
    assert {w.variant[0] for w in worlds} == {v[0] for v in model.VARIANTS}
    assert total["discarded"] >= 2  # hb_discard_appended with results live
    assert (_lib._lib, _lib._lib_exp) == before  # (nothing was loaded for it; another test of the same process may have)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_interleaved_calls_against_the_model(gpu_ctx_factory, seed):
    model.run(seed, gpu_ctx_factory)
