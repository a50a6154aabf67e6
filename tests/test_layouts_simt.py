"""tests/test_layouts.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the plan-reading operators under non-default
plan layouts, checked on the CPU against their host restatements.  The interpreter takes the first 25 contexts of the case list (about
a minute; conditions (a) to (f) of tests/operator_cases.py all occur among them), the first 8 contexts of the live-first list (about
20 s; every kind twice, condition (g) in four and (h) in three of them; HB_SIMT_FULL=1: all 16) and the crafted fan case; the condition and
cap tests count over the whole lists either way, since they need the host planner and the restatements only."""
import os

from tests.simt_wrap import run, simt_lib  # noqa: F401  (simt_lib is the fixture)

PREFIX = 25
LIVE_PREFIX = 16 if os.environ.get("HB_SIMT_FULL") == "1" else 8


def test_layouts_under_the_interpreter(simt_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("HB_LAYOUT_CASES", str(PREFIX))
    monkeypatch.setenv("HB_LIVE_LAYOUT_CASES", str(LIVE_PREFIX))
    run(simt_lib, "test_layouts.py", None, None)


def test_layout_fan_case_in_shuffled_order(simt_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("HB_LAYOUT_CASES", "3")
    monkeypatch.setenv("HB_LIVE_LAYOUT_CASES", "0")
    run(simt_lib, "test_layouts.py", "shuffle:7", "test_fan or 02-stars")
