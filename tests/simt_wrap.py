"""What the test_*_simt.py wrappers share: the interpreted build of the library (tests/simt, see tests/test_simt.py) and one run of a
GPU test file against it in a child process, in the default workgroup / lane order or in a given one."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMT = os.path.join(ROOT, "tests", "simt")
LIB = os.path.join(SIMT, "_build", "libhyperball_simt.so")


@pytest.fixture(scope="module")
def simt_lib():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and not os.environ.get("CLANG"):
        pytest.skip("no clang++ to build the interpreted library with")
    subprocess.check_call(["make", "-s", "-j8", "-C", SIMT])
    assert os.path.exists(LIB)
    return LIB


def run(lib, test_file, order=None, select=None):
    """pytest -m gpu on tests/<test_file> with the interpreted library; `select` is a -k expression"""
    env = dict(os.environ, HB_LIB_PATH=lib, HB_ALLOW_SIMT_INTERPRETER="1", PYTHONPATH=ROOT)
    if order:
        env.update(HB_SIMT_ORDER=order, HB_SIMT_THREADS="3")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", test_file), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"]
    if select:
        cmd += ["-k", select]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=1700)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail
