"""The exact tests of the align_corners=True bilinear kernels (tests/test_exact_resample_ac_gpu.py: the ssa_resize_* entry
points, the autograd Functions, eval_tail.resize_tensor) on the CPU EMULATION build of the kernel sources, for both storage
types -- as tests/test_conv5x5_emu_cpu.py runs the 5x5 conv -- so that the default CPU suite checks the index arithmetic
of the second rule on every route: the candidate ranges and their scale-0 regime, the window sizing of the tiled
backward, the batched loads of the separable pair and the argument checks.  The six grid-stride cases (2 M threads and
more) skip under emulation and run on the device."""
import os
import re
import subprocess
import sys

import pytest

import resample_ac_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every case of the four tables, the twelve dispatch cases, six image resizes and the five single tests
PASSED = len(AC.FWD_EXACT) + len(AC.BWD_EXACT) + len(AC.SEP_EXACT) + len(AC.BOUNDED) + 12 + 6 + 5


def test_emulated_count():
    assert (len(AC.FWD_EXACT), len(AC.BWD_EXACT), len(AC.SEP_EXACT), len(AC.BOUNDED)) == (38, 51, 19, 22) and PASSED == 153


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_exact_resample_ac_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_exact_resample_ac_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == PASSED and "failed" not in tail, tail
