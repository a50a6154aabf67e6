"""tests/test_ampc_state.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the interleaved calls of tests/ampc_model.py
against the host layer of hb_ampc.hip and every AMPC kernel on the CPU, in the default workgroup / lane order and - a slice of the seed
list - in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_ampc_state_sequences_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_ampc_state.py")


def test_ampc_state_sequences_in_shuffled_order(simt_lib):  # noqa: F811
    # what depends on which lane or workgroup comes first: the slot a new key gets, the atomics of the filters, the counts
    run(simt_lib, "test_ampc_state.py", "shuffle:7", "101 or 104 or 109 or 114")
