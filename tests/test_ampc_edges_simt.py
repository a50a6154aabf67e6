"""tests/test_ampc_edges.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_ampc_edges.hip.h and their driver in hb_ampc.hip, checked on the CPU against the restatement of tests/ampc_ref.py,
in the default workgroup / lane order and in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_ampc_edge_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_ampc_edges.py")


def test_ampc_edge_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # the fused counter fold and the distance fold with its group actions: what depends on which lane or workgroup comes first
    run(simt_lib, "test_ampc_edges.py", "shuffle:7", "test_update_counters_group_lengths or test_update_distances_group_lengths_and_actions")
