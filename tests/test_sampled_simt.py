"""tests/test_sampled_harmonic.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the sampled-BFS kernels of
stract_amd/csrc/hb_sample.hip.h and their driver, checked on the CPU against the host restatement, in the default workgroup / lane
order and in a shuffled one.  The C2-size case stays on the GPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)

SELECT = "not test_c2"  # (j) needs a 20 M-edge graph: GPU only


def test_sampled_kernels_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_sampled_harmonic.py", None, SELECT)


def test_sampled_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_sampled_harmonic.py", "shuffle:7", "test_fixture_graphs or test_lcg_graph or test_batch_boundaries or test_layout_variants")
