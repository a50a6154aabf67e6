"""tests/test_extreme_registers.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the `big` branch of every copy of the
epilogue, saturated sizes, Kahan terms of about 2^64, registers of 48..58 and 65 through pass 0's jp entries and the six-bit wire,
checked on the CPU against the oracle, in the default workgroup / lane order and in a shuffled one."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_extreme_registers_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_extreme_registers.py")


def test_extreme_registers_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_extreme_registers.py", "shuffle:7")
