"""The device evaluation tail, as far as it can be checked without a GPU:
  * the kernel tests of tests/test_eval_tail_gpu.py on the CPU emulation of the kernel sources (SSA_EMU=1, the way
    tests/test_emu_selected_cpu.py runs its selection) -- index arithmetic, LDS layout and barrier structure of
    ssa_eval_tail and the host side of eval_minibatch;
  * tests/evaltail_ref.py, the restatement those tests trust, against tests/golden/evaltail_golden.pt, recorded from the
    reference's own eval_minibatch by tests/golden/make_golden_evaltail.py;
  * argument validation of ssa_eval_tail and the `utils.trnval_utils` registration of dropin.install()."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import evaltail_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_tests_pass_on_the_emulated_kernels():
    env = dict(os.environ, SSA_EMU="1")
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_eval_tail_gpu.py"), "-q", "-x",
                        "-m", "gpu", "-k", "not full_size", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "tests/test_eval_tail_gpu.py under SSA_EMU=1:\n%s\n%s" % (tail, r.stderr[-2000:])
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


def _golden_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_golden_evaltail as M
    finally:
        sys.path.pop(0)
    return M


@pytest.mark.parametrize("name", ["mscale19", "mscale65", "multi19", "plain19"])
def test_restatement_reproduces_the_reference_fixture(name):
    M = _golden_cases()
    rec = torch.load(os.path.join(ROOT, "tests", "golden", "evaltail_golden.pt"))[name]
    C, ignore, mscale, net, data, args = M.build_case(name)
    meter = R.Meter()
    assets, hist = R.eval_minibatch(data, net, R.CpuCrossEntropyLoss2d(ignore), meter, True, args, 1, C, ignore, mscale)
    assert list(assets.keys()) == rec["keys"]
    for k, v in assets.items():
        if k == "prob_mask":
            assert isinstance(v, torch.Tensor) and v.dtype == torch.float32
            assert float((v - rec[k]).abs().max()) <= 1e-6
        elif "attn_" in k:
            assert tuple(v.shape) == rec[k + ".shape"]
        else:
            assert isinstance(v, np.ndarray) and v.dtype == np.int64, k
            assert np.array_equal(v, rec[k].numpy().astype(np.int64)), k
    assert hist.dtype == np.int64 and np.array_equal(hist, rec["hist"].numpy())
    assert meter.count == rec["count"] and abs(meter.avg - rec["loss"]) <= 1e-6 * max(1.0, abs(rec["loss"]))


def test_eval_tail_rejects_bad_arguments_without_gpu():
    """ssa_eval_tail returns SSA_EINVAL before it touches the device."""
    from semseg_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)           # a non-null address; never dereferenced
    p = ctypes.c_void_p(ctypes.addressof(buf))
    one = (ctypes.c_void_p * 8)(*[p.value] * 8)
    nine = (ctypes.c_void_p * 9)(*[p.value] * 9)
    flips = (ctypes.c_int * 9)()

    def call(srcs=one, n=1, ld=19, C=19, labels=None, pred=p, err=None, hist=None, loss=None, avg=None, ds=1.0, df=1.0):
        return L.ssa_eval_tail(srcs, flips, n, ld, 1, 4, 4, C, labels, 255, ds, df, pred, None, err, hist, loss, avg, None)
    assert call(n=0) == -1 and call(srcs=nine, n=9) == -1                    # 1 .. 8 sources
    assert call(C=129, ld=129) == -1 and call(C=0, ld=0) == -1               # 1 .. 128 classes
    assert call(ld=18) == -1                                                 # ld < C
    assert call(srcs=(ctypes.c_void_p * 8)(p.value, None), n=2) == -1        # a null source
    assert call(srcs=None) == -1
    assert call(err=p) == -1 and call(hist=p) == -1 and call(loss=p) == -1   # need labels
    assert call(pred=None) == -1                                             # nothing asked for
    assert call(ds=0.0) == -1 and call(df=-1.0) == -1


def test_install_registers_trnval_utils_only_on_request():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "semantic-segmentation_amd"), ROOT]))
    code = """
import sys
import semseg_amd.dropin as dropin
dropin.install()
assert "utils.trnval_utils" not in sys.modules
dropin.install(device_eval_tail=True)
import semseg_amd.utils as U
m = sys.modules["utils.trnval_utils"]
assert m.eval_minibatch is U.eval_minibatch and m.flip_tensor is U.flip_tensor and m.resize_tensor is U.resize_tensor
try:
    m.validate_topn(None, None, None, None, 0, None)
except NotImplementedError as e:
    assert "run_minibatch" in str(e)
else:
    raise AssertionError("validate_topn did not raise")
from semseg_amd.config import cfg
assert cfg.MODEL.MSCALE is False
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
