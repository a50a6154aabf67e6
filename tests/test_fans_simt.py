"""tests/test_fans.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the walk kernels of hb_bfs.hip.h,
hb_betweenness.hip.h, hb_similarity.hip.h, hb_sample.hip.h and hb_walk.hip.h on lists at, just under and just over every list-length
switch, checked on the CPU against closed forms, in the default workgroup / lane order and in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_fans_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_fans.py")


def test_fans_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_fans.py", "shuffle:7")
