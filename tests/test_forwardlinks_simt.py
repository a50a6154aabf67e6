"""tests/test_forwardlinks.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the forward kernels of
stract_amd/csrc/hb_links.hip.h and their driver, checked on the CPU against the host restatement, in the default workgroup / lane order
and in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_forwardlinks_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_forwardlinks.py", None, None)


def test_forwardlinks_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # the degree counters, the histograms and the emit cursors are where workgroup order could leak into a result
    run(simt_lib, "test_forwardlinks.py", "shuffle:7", "test_long or test_self_links or test_equal_keys or test_u64_max or test_batches or test_ascent")
