"""tests/test_ampc_approx.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_ampc_fold.hip.h and their drivers in hb_ampc.hip, checked on the CPU against the restatement of
tests/ampc_approx_ref.py, in the default workgroup / lane order and - the fold and the sketch - in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_ampc_approx_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_ampc_approx.py")


def test_ampc_approx_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # what depends on which lane or workgroup comes first: the entry numbers the fold's inserts get, the counts, the sketch's maxima
    run(simt_lib, "test_ampc_approx.py", "shuffle:7", "test_fold or test_three_folds or test_node_sketch or test_run_approx")
