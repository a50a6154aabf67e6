"""tests/test_context_state.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the interleaved calls of
tests/context_model.py against the host layer of hb_api.hip and every kernel of the context on the CPU, in the default workgroup / lane
order and - a slice of the seed list - in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_context_state_sequences_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_context_state.py")


def test_context_state_sequences_in_shuffled_order(simt_lib):  # noqa: F811
    # what depends on which lane or workgroup comes first: the selects of the list builder, the atomics of the walks
    run(simt_lib, "test_context_state.py", "shuffle:7", "601 or 605 or 610")
