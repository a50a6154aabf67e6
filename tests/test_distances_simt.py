"""tests/test_distances.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the BFS kernels of stract_amd/csrc/hb_bfs.hip.h
and their driver, checked on the CPU against the host restatement, in the default workgroup / lane order and in a shuffled one.  The
C2-size case stays on the GPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)

SELECT = "not test_c2"  # (11) needs a 20 M-edge graph: GPU only


def test_distance_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_distances.py", None, SELECT)


def test_distance_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    # (2), (4) and (5): the fixture / lcg graphs, the deep and the wide graph, each with the default and both forced steps
    run(simt_lib, "test_distances.py", "shuffle:7", "test_fixture_graphs or test_lcg_graph or test_long_tail or test_star")
