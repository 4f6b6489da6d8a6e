"""The exact tests of the implicit-GEMM gather (tests/test_igemm_addressing_gpu.py) on the CPU EMULATION of the kernels
(tools/emu: the unchanged kernel sources compiled for the host), in a subprocess with SSA_EMU=1, for both storage
builds -- the way tests/test_emu_selected_cpu.py runs its selection.  The cases are small enough that all of them run in
seconds, so the row offsets, tap masks and the tap cursor of csrc/conv_igemm.hip are checked bit for bit by the default
CPU suite."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = "tests/test_igemm_addressing_gpu.py"
# (a) at six tile configurations, (b) (c) (d) (g) (h) (i) at two, (e) at two strides times two, (f) once
MIN_PASSED = 23


def _run(extra):
    env = dict(os.environ, SSA_EMU="1", **extra)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, PATH), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "%s under SSA_EMU=1 %r:\n%s\n%s" % (PATH, extra, tail, r.stderr[-2000:])
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED, "%s ran %s tests, expected >= %d:\n%s" % (
        PATH, m.group(1) if m else "no", MIN_PASSED, tail)


def test_igemm_addressing_on_the_emulated_kernels_bf16():
    _run({})


def test_igemm_addressing_on_the_emulated_kernels_fp16():
    _run({"SSA_ACT_DTYPE": "fp16"})
