"""tests/test_links.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of stract_amd/csrc/hb_links.hip.h and
their driver, checked on the CPU against the host restatement, in the default workgroup / lane order and in a shuffled one.  The C2-size
case stays on the GPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_links_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_links.py", None, "not test_c2")


def test_links_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # cursors and histograms are where workgroup order could leak into a result: the list lengths, the self links, the ties, the batches
    run(simt_lib, "test_links.py", "shuffle:7", "test_list_lengths or test_self_links or test_ties or test_u64_max or test_batches")
