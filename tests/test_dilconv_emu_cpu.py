"""The exact tests of the rectangular-dilation 3x3 conv family (tests/test_exact_dilconv_gpu.py: ssa_dilconv3x3,
ssa_dilconv3x3_wgrad) on the CPU EMULATION build of the kernel sources, for both storage types -- as
tests/test_gconv_emu_cpu.py runs the grouped family -- so that the default CPU suite checks the shifted-window addressing
and its per-pixel validity, the per-tile tap list, the fragment order of the packed filter (forward and data gradient),
the register double buffer's step arithmetic, the staged epilogue and its statistics, the grouped launch, the staged
weight gradient with its ordered reduce, and the argument checks.  The emulation runs EVERY case (none is left to the
device alone)."""
import os
import re
import subprocess
import sys

import pytest

import dilconv_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the regime mirror, the rounding census, every forward / data-gradient / layout case, the grouped launch, every
# weight-gradient case, the argument checks
MIN_PASSED = 2 + len(DC.CASES) + 1 + len(DC.WG_CASES) + 1


def test_emulated_case_count():
    assert (len(DC.CASES), len(DC.WG_CASES), MIN_PASSED) == (12, 4, 20)


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_exact_dilconv_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_exact_dilconv_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail and "skipped" not in tail, tail
