"""tools/emu/build.sh run by several processes at once (every rank of a multi-process emulated test calls it through
tests/emu_util.py) must never leave a moment in which the library is missing: a rank that loaded it in such a moment
died, and its peer failed in a collective with "Connection closed by peer"."""
import os
import subprocess
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_concurrent_rebuilds_keep_the_library_in_place():
    from emu_util import build_emu
    lib = build_emu()
    obj = os.path.join(os.path.dirname(lib), "emu_runtime.o")
    later = os.path.getmtime(lib) + 1.0
    os.utime(obj, (later, later))                 # an object newer than the library: both runs below relink
    script = os.path.join(ROOT, "tools", "emu", "build.sh")
    procs = [subprocess.Popen(["sh", script], stdout=subprocess.DEVNULL) for _ in range(2)]
    missing = 0
    while any(p.poll() is None for p in procs):
        missing += not os.path.exists(lib)
        time.sleep(0.001)
    assert [p.returncode for p in procs] == [0, 0]
    assert missing == 0, "the library was missing in %d polls during the rebuilds" % missing
    assert os.path.getmtime(lib) >= later         # relinked, not skipped
    assert not [f for f in os.listdir(os.path.dirname(lib)) if ".tmp." in f]
    # up to date: a further run does not touch the library
    before = os.stat(lib).st_mtime_ns
    subprocess.check_call(["sh", script], stdout=subprocess.DEVNULL)
    assert os.stat(lib).st_mtime_ns == before
