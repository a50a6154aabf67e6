"""tests/test_similarity.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_similarity.hip.h and their driver, checked on the CPU against the host restatement, in the default workgroup / lane
order and in a shuffled one.  The C2-size case stays on the GPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)

SELECT = "not test_c2"  # needs a 20 M-edge graph: GPU only


def test_similarity_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_similarity.py", None, SELECT)


def test_similarity_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # the known answer, the slot packing, the star, the three modes and the wide ids, each with the default and both forced modes
    run(simt_lib, "test_similarity.py", "shuffle:7", "test_known_answer or test_lcg_entry_counts or test_star or test_modes or test_wide")
