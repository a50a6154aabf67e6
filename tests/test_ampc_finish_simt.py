"""tests/test_ampc_finish.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_ampc_finish.hip.h, the device forms of hb_ingest.hip's sorts and their drivers in hb_ampc.hip, checked on the CPU against
tests/ampc_finish_ref.py, in the default workgroup / lane order and - the finish and the top lists - in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_ampc_finish_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_ampc_finish.py")


def test_ampc_finish_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # the entry numbers of a table's keys depend on which lane claims its slot first; ids, values, ranks and top lists must not
    run(simt_lib, "test_ampc_finish.py", "shuffle:7", "test_finish or test_id_order or test_300 or test_two_tie or test_special or test_every_combination")
