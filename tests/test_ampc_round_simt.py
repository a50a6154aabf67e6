"""tests/test_ampc_round.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_ampc_round.hip.h and their driver in hb_ampc.hip, checked on the CPU against the restatement of tests/ampc_round_ref.py,
in the default workgroup / lane order and - the chunk-boundary tests and the filter-update tests - in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_ampc_round_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_ampc_round.py")


def test_ampc_round_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # what depends on which lane or workgroup comes first: the atomics of the filter update and of the exact set's index, the counts
    run(simt_lib, "test_ampc_round.py", "shuffle:7",
        "test_round_counters or test_round_distances or test_union or test_exact_set or test_bloom_filter_against_the_model or test_setup_counters")
