"""tests/test_early_exit.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): every pass with the early exit forced, off
and under the default rule against the oracle, the count of rows that left early against the host model of the launched rounds, the
rule and the contexts outside the gate - checked on the CPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_early_exit_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_early_exit.py", None, None)


def test_early_exit_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_early_exit.py", "shuffle:5", "hub or last_source")
