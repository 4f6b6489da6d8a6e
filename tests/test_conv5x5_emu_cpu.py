"""The exact tests of the 5x5 conv kernel (tests/test_exact_conv5x5_gpu.py: ssa_conv2d_halo5) on the CPU EMULATION build of
the kernel sources, for both storage types -- as tests/test_dwconv_emu_cpu.py runs the depthwise family -- so that the
default CPU suite checks the halo addressing and its edge masks, the swizzled fragment reads, the filter ring's k-step
arithmetic, the chunk double buffer, the partial n-block group and the argument checks.  The emulation runs the cases of
at most two chunks plus the first data-gradient case (conv5x5_cases.EMU_IDS); the cases of five and six chunks repeat
the same buffer hand-over more often and run on the device."""
import os
import re
import subprocess
import sys

import pytest

import conv5x5_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_case_list():
    assert CC.EMU_IDS == ["c64", "c128", "c96", "n40", "n40bias", "sliced", "d320"]


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_exact_conv5x5_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    sel = " or ".join("test_exact_conv5x5[%s]" % i for i in CC.EMU_IDS)
    sel += " or regimes or need_rounding or argument_checks"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_exact_conv5x5_gpu.py"), "-q", "-m", "gpu",
                        "-k", sel, "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == len(CC.EMU_IDS) + 3 and "failed" not in tail, tail
