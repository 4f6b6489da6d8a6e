"""The exact tests of the pre-activation passes (tests/test_exact_preact_gpu.py: ssa_add_bn_stats, ssa_bn_bwd_apply_add)
on the CPU EMULATION build of the kernel sources, for both storage types -- as tests/test_emu_selected_cpu.py runs the
other exact kernel tests, so that the default CPU suite checks index arithmetic, masking, the block reduction and the
argument checks of the two kernels.  The case of 17 M elements skips under emulation (the GPU runs it)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 4 of the 5 cases of each kernel, the regime mirror, the random-operand case, the argument checks and the unbuilt forms
MIN_PASSED = 12


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_exact_preact_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_exact_preact_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
