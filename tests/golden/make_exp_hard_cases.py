#!/usr/bin/env python3
"""Generate tests/golden/exp_hard_cases.txt: arguments of csrc/swd_libm.h's exp whose RESULT changes when the polynomial
coefficient C2 of swd_exp_from changes by one ulp, up or down.

Why: the polynomial's terms are small against the result (|r| <= ln2 / 256, so C2 r^2 <= 3.7e-6), and one ulp of C2 moves the value
before the last rounding by at most 4e-22 of the result: the rounded result changes for about one argument in a million.  Random
arguments, or arguments on the branch thresholds, do not notice such a change (none of the 217 564 of tests/libm_args.py did, 2 of
the 3 000 000 of tests/csrc/libm_check.c did); the arguments found here, whose value before the last rounding lies that close to a
rounding boundary, do.  They are the cases where the device's evaluation has the least room: a different order of two operations
or a fused pair shows on them first.  (One ulp of C3 shows a thousand times less often still, of C4 and C5 practically never: such
a change is below what any list of arguments resolves.)

How: the header is copied to a temporary directory twice with the C2 literal moved one ulp up / down, tests/csrc/libm_check.c is
built against each copy and against the header itself, and random arguments (the classes of tests/libm_args.py over the whole range
of finite results, and [-40, 0], the arguments exp sees inside logaddexp) are kept where a copy's result differs.  Deterministic:
seeded, the first PER_CLASS finds of each class and direction.  No reference source is involved.
"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "slidingwindowdecoder_amd", "csrc")
C2 = "0x1.ffffffffffdbdp-2"
PER_CLASS = 32
CHUNK = 1 << 22


def build(c2, d):
    src = open(os.path.join(CSRC, "swd_libm.h")).read()
    assert src.count("C2 = " + C2) == 1
    os.makedirs(d)
    open(os.path.join(d, "swd_libm.h"), "w").write(src.replace("C2 = " + C2, "C2 = " + c2))
    so = os.path.join(d, "libm_check.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", d, "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "libm_check.c"),
                           "-o", so, "-lm"])
    L = C.CDLL(so)
    L.swd_eval_header.restype = C.c_int
    L.swd_eval_header.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]

    def ev(x):
        out = np.empty_like(x)
        assert L.swd_eval_header(0, x.size, x.ctypes.data, None, out.ctypes.data) == 0
        return out
    return ev


def main():
    c2 = float.fromhex(C2)
    tmp = tempfile.mkdtemp(prefix="swd_exp_hard_")
    evs = [build(C2, os.path.join(tmp, "same"))] + [build(float(np.nextafter(c2, t)).hex(), os.path.join(tmp, n)) for t, n in ((1.0, "up"), (0.0, "down"))]
    rng = np.random.default_rng(0xC2)
    classes = [lambda n: (rng.random(n) - 0.5) * 100.0, lambda n: -rng.random(n) * 708.0, lambda n: rng.random(n) * 709.0, lambda n: -rng.random(n) * 40.0]
    found = []
    for ci, draw in enumerate(classes):
        got = [[], []]
        while min(len(g) for g in got) < PER_CLASS:
            x = draw(CHUNK)
            want = evs[0](x)
            for k in (0, 1):
                got[k] += x[evs[1 + k](x) != want].tolist()
        print(f"class {ci}: {[len(g) for g in got]} found", file=sys.stderr)
        found += got[0][:PER_CLASS] + got[1][:PER_CLASS]
    path = os.path.join(HERE, "exp_hard_cases.txt")
    with open(path, "w") as f:
        f.write("# arguments whose exp changes when C2 of swd_exp_from moves by one ulp (tests/golden/make_exp_hard_cases.py)\n")
        for v in found:
            f.write(float(v).hex() + "\n")
    print(f"wrote {len(found)} arguments")


if __name__ == "__main__":
    main()
