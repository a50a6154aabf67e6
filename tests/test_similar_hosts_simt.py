"""tests/test_similar_hosts.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_similar.hip.h and their driver, checked on the CPU against the literal restatement, in the default workgroup / lane
order and in a shuffled one.  The C2-size case stays on the GPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_similar_hosts_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_similar_hosts.py", None, "not test_c2")


def test_similar_hosts_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # the claim of a source, the counters, the touched list and the lists' cursors are where workgroup order could leak into a result
    run(simt_lib, "test_similar_hosts.py", "shuffle:7", "test_filter_switch or test_in_list_cuts or test_duplicate or test_the_gated")
