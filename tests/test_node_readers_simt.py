"""tests/test_node_readers.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the readers of hb_distances, hb_betweenness
and hb_nearest_seed and the two _top readers, one C entry point at a time, on the CPU - where the "device" memory is poisoned host
memory - before they reach a card."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_node_readers_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_node_readers.py")
