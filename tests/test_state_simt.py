"""tests/test_state.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the five calls that share the device rows in
every order on one context, and what each leaves readable, on the CPU - in the default workgroup / lane order and in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_state_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_state.py")


def test_state_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_state.py", "shuffle:7")
