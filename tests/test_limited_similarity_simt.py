"""tests/test_limited_similarity.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_similarity_limit.hip.h, the list builder they are fed by and their driver, checked on the CPU against the host
restatement, in the default workgroup / lane order and in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_limited_similarity_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_limited_similarity.py")


def test_limited_similarity_in_shuffled_order(simt_lib):  # noqa: F811
    # the level-1 bits and the counters of the list-count kernel are atomic: the cut at its edge, the self links, the modes and batches
    # and the R-MAT graph once more in another order
    run(simt_lib, "test_limited_similarity.py", "shuffle:7", "test_cut_at_its_edge or test_self_links or test_modes_and_batches or test_c1_rmat")
