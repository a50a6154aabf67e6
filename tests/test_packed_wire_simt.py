"""tests/test_packed_wire.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the three kernels of HB_FLAG_PACKED_WIRE
against the restated bit stream, the packed exchanges between logical ranks against the oracle after every pass with their booked
bytes, the flag off, the refusals and the one-rank communicator - checked on the CPU.  The multi-process test needs the real device."""
from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)


def test_packed_wire_under_the_interpreter(simt_lib):  # noqa: F811
    run(simt_lib, "test_packed_wire.py", None, "not multi_process")


def test_packed_wire_kernels_in_shuffled_order(simt_lib):  # noqa: F811
    run(simt_lib, "test_packed_wire.py", "shuffle:5", "every_value or tails or straddles")
