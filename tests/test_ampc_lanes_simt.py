"""tests/test_ampc_lanes.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_ampc_lanes.hip.h and their drivers in hb_ampc.hip, checked on the CPU against the restatement of
tests/ampc_lanes_ref.py, in the default workgroup / lane order and - the round step, the fold and the drivers - in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_ampc_lanes_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_ampc_lanes.py")


def test_ampc_lanes_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # what depends on which lane or workgroup comes first: the entry numbers the upsert's and the fold's inserts get, the counts, the
    # members of new_changed - never a row or a sum
    run(simt_lib, "test_ampc_lanes.py", "shuffle:7", "test_round or test_fold or test_three_zero or test_run_ or test_batches")
