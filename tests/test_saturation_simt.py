"""tests/test_saturation.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the saturation bound, the bitmap after every
dense pass, every pass against the oracle with saturated rows and their hub chunks skipped, on against off and the contexts outside
the gate - checked on the CPU."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_saturation_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_saturation.py", None, None)


def test_saturation_passes_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_saturation.py", "shuffle:5", "per_pass and (hubs or ring65)")
