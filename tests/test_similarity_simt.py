"""tests/test_similarity.py under the SIMT interpreter (tests/simt, see tests/test_simt.py): the kernels of
stract_amd/csrc/hb_similarity.hip.h and their driver, checked on the CPU against the host restatement, in the default workgroup / lane
order and in a shuffled one.  The C2-size case stays on the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMT = os.path.join(ROOT, "tests", "simt")
LIB = os.path.join(SIMT, "_build", "libhyperball_simt.so")
SELECT = "not test_c2"  # needs a 20 M-edge graph: GPU only


@pytest.fixture(scope="module")
def simt_lib():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and not os.environ.get("CLANG"):
        pytest.skip("no clang++ to build the interpreted library with")
    subprocess.check_call(["make", "-s", "-j8", "-C", SIMT])
    assert os.path.exists(LIB)
    return LIB


def _run(lib, order, select):
    env = dict(os.environ, HB_LIB_PATH=lib, HB_ALLOW_SIMT_INTERPRETER="1", PYTHONPATH=ROOT)
    if order:
        env.update(HB_SIMT_ORDER=order, HB_SIMT_THREADS="3")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_similarity.py"), "-m", "gpu", "-q", "-x",
                        "-k", select, "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1700)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail


def test_similarity_kernels_under_the_interpreter(simt_lib):
    _run(simt_lib, None, SELECT)


def test_similarity_kernels_in_shuffled_order(simt_lib):
    # the known answer, the slot packing, the star, the three modes and the wide ids, each with the default and both forced modes
    _run(simt_lib, "shuffle:7", "test_known_answer or test_lcg_entry_counts or test_star or test_modes or test_wide")
