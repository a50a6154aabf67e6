"""tests/test_live_first.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the live-first device order - both
planners, every pass against the oracle in every pass mode with the order forced on, on against off, the contexts that ignore the
option and the plan-reading operators - checked on the CPU (about half a minute)."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_live_first_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_live_first.py", None, None)


def test_live_first_passes_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_live_first.py", "shuffle:5", "per_pass and (fan64 or fan65 or all_sources_dead)")
