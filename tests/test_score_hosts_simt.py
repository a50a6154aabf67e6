"""tests/test_score_hosts.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_score.hip.h, the BitVec body they share with hb_similar.hip.h, the list builder they are fed by and their driver,
checked on the CPU against the host restatement and against the lookup route, in the default workgroup / lane order and in a shuffled
one.  The C2-size case stays on the GPU, and so does the call that shows 262144 distinct hosts allowed: it would run that many workgroups
of the BitVec kernel through the interpreter (the refusal of 262145 runs here)."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_score_hosts_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_score_hosts.py", None, "not test_c2 and not test_262144_distinct_hosts_are_allowed")


def test_score_hosts_in_shuffled_order(simt_lib):  # noqa: F811
    # the pair counters are atomic and the pair words of a piece are written by one wave each: the list lengths and the request counts,
    # plain and under small pieces and the links debug flags, and the long anchor list once more in another workgroup and lane order
    run(simt_lib, "test_score_hosts.py", "shuffle:7", "test_list_lengths or test_request_counts or test_a_piece_boundary")
