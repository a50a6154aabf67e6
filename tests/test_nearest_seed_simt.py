"""tests/test_nearest_seed.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_nearest_seed.hip.h and their driver, checked on the CPU against the host restatement, in the default workgroup /
lane order and in a shuffled one.  The C2-size cases stay on the GPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)

SELECT = "not test_c2"  # a 20 M-edge graph and a 2^20-node one: GPU only


def test_nearest_seed_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_nearest_seed.py", None, SELECT)


def test_nearest_seed_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # the list lengths, the self links and the ties: what depends on which lane or workgroup comes first
    run(simt_lib, "test_nearest_seed.py", "shuffle:7", "test_list_lengths or test_self_link or test_ties")
