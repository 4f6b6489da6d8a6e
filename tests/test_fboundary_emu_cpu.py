"""The boundary F-score tests (tests/test_fboundary_gpu.py: the kernels of csrc/fboundary.hip through the C ABI, through
boundary_counts, eval_mask_boundary, BoundaryMeter and eval_minibatch) on the CPU EMULATION build of the kernel sources,
for both storage builds -- as tests/test_relaxloss_emu_cpu.py runs the label relaxation tests -- so that the default
CPU suite checks the quad rules, the tile seams and halos of the match kernel, the disk's edge, the label rules and
every integer count against the restatement and the golden data of the real reference, and the argument checks.  The
full-size run skips under emulation (the GPU runs it)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 15 cases through the C ABI, 15 through boundary_counts, 3 non-contiguous, 15 through eval_mask_boundary, arguments,
# launch budget, eval_minibatch, the torch composition
MIN_PASSED = 52


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_fboundary_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_fboundary_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
