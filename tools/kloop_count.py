#!/usr/bin/env python
"""Instruction mix of a kernel's main loop, from the assembly `hipcc -S --cuda-device-only` writes.

python tools/kloop_count.py <file.s> <substring of the mangled kernel name> [more substrings ...]

The main loop is the innermost-closed span (label .. backward branch to it) that holds the most MFMAs.  Printed: the
span's VALU / SALU / waitcnt / memory / LDS / MFMA counts, and the kernel's register use from its .vgpr_count notes."""
import re
import sys


def functions(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                yield name, body
                name = None
            else:
                body.append(line.strip())


def main_loop(body):
    labels = {}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"^s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels:
            lo = labels[m.group(1)]
            n = sum(1 for x in body[lo:i] if x.startswith("v_mfma"))
            if best is None or n > best[0]:
                best = (n, lo, i + 1)
    return best


def classify(span):
    c = dict(valu=0, salu=0, waitcnt=0, gload=0, gstore=0, ds_write=0, ds_read=0, mfma=0, v_cmp=0, v_cndmask=0, v_mul=0, branch=0)
    for l in span:
        op = l.split()[0] if l and not l.startswith((".", ";")) and not l.endswith(":") else None
        if op is None:
            continue
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("s_waitcnt"):
            c["waitcnt"] += 1
        elif op.startswith(("global_load", "buffer_load")):
            c["gload"] += 1
        elif op.startswith(("global_store", "buffer_store")):
            c["gstore"] += 1
        elif op.startswith("ds_write") or op.startswith("ds_store"):
            c["ds_write"] += 1
        elif op.startswith("ds_read") or op.startswith("ds_load"):
            c["ds_read"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
            c["salu"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op.startswith("v_cmp"):
                c["v_cmp"] += 1
            if op.startswith("v_cndmask"):
                c["v_cndmask"] += 1
            if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64", "v_mul_u32", "v_mad_u32", "v_mad_i32")):
                c["v_mul"] += 1
        elif op.startswith("s_") and op not in ("s_nop", "s_barrier", "s_endpgm"):
            c["salu"] += 1
    return c


def main():
    path, keys = sys.argv[1], sys.argv[2:]
    text = open(path).read()
    for name, body in functions(path):
        if not all(k in name for k in keys):
            continue
        best = main_loop(body)
        if best is None:
            continue
        n, lo, hi = best
        c = classify(body[lo:hi])
        m = re.search(r"\.name:\s+%s\b.*?\.vgpr_count:\s+(\d+)" % re.escape(name), text, re.S)
        a = re.search(r"\.agpr_count:\s+(\d+)(?:(?!\.agpr_count).)*?\.name:\s+%s\b" % re.escape(name), text, re.S)
        print("%s\n  main loop: %d lines, %s\n  vgpr_count %s agpr_count %s" % (
            name, hi - lo, " ".join("%s=%d" % kv for kv in c.items()), m.group(1) if m else "?", a.group(1) if a else "?"))


if __name__ == "__main__":
    main()
