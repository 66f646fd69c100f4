"""csrc/swd_libm.h (the device's exp / log1p, used by the quaternary decoder) against the host C library, bit for
bit.  The reference's bp4_osd calls glibc's exp and log1p; its goldens were recorded on an FMA-capable x86-64 with
glibc 2.35, whose exp has an FMA build -- the restatement follows that build, so the comparison needs such a host."""
import ctypes as C
import os
import platform
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return platform.machine() == "x86_64" and " fma " in f.read().replace("\n", " ")
    except OSError:
        return False


@pytest.fixture(scope="module")
def shim():
    if not _host_has_fma():
        pytest.skip("host C library would select its non-FMA exp here; the restatement follows the FMA build")
    d = tempfile.mkdtemp(prefix="swd_libm_")
    so = os.path.join(d, "libm_check.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "slidingwindowdecoder_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "libm_check.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    for f in (L.swd_check_exp, L.swd_check_log1p):
        f.restype = C.c_long
        f.argtypes = [C.c_long, C.c_uint64, C.POINTER(C.c_double)]
    return L


def test_exp_table_is_current():
    """the committed table equals what scripts/gen_exp_table.py derives"""
    path = os.path.join(ROOT, "slidingwindowdecoder_amd", "csrc", "swd_exp_table.h")
    with tempfile.TemporaryDirectory(prefix="swd_exp_") as d:  # never touches the tracked header (its mtime drives make)
        fresh = os.path.join(d, "swd_exp_table.h")
        subprocess.check_call(["python3", os.path.join(ROOT, "scripts", "gen_exp_table.py"), fresh], stdout=subprocess.DEVNULL)
        assert open(fresh).read() == open(path).read()


def test_exp_matches_host_libm(shim):
    x = C.c_double(0.0)
    bad = shim.swd_check_exp(3_000_000, 12345, C.byref(x))
    assert bad == 0, f"{bad} arguments differ, first {x.value!r}"


def test_log1p_matches_host_libm(shim):
    x = C.c_double(0.0)
    bad = shim.swd_check_log1p(3_000_000, 999, C.byref(x))
    assert bad == 0, f"{bad} arguments differ, first {x.value!r}"


def test_args_are_what_they_promise():
    """tests/libm_args.py: deterministic, at most 2^18 arguments per op, every listed threshold with its 64 neighbours either side"""
    from tests import libm_args as A
    for op in range(7):
        x, y = A.args(op)
        x2, y2 = A.args(op)
        assert 200_000 < x.size <= 1 << 18 and x.tobytes() == x2.tobytes() and (y is None) == (op not in (4, 6))
        if y is not None:
            assert y.tobytes() == y2.tobytes()
    nb = A.around(512.0)
    assert nb.size == 129 and nb[64] == 512.0 and (np.diff(nb) > 0).all() and nb[0] == 512.0 - 64 * 2.0 ** -44 and nb[-1] == 512.0 + 64 * 2.0 ** -43
    for op, ts in ((0, A.EXP_THRESHOLDS), (2, A.LOG1P_THRESHOLDS), (3, A.LOG1PEXP_THRESHOLDS + A.EXP_THRESHOLDS)):
        have = set(A.args(op)[0].view(np.uint64).tolist())
        for t in ts:
            for s in (1.0, -1.0):
                assert set((s * A.around(t)).view(np.uint64).tolist()) <= have, (op, t, s)
    hard = A.exp_hard_cases()
    assert hard.size == 256 and (hard < 0).sum() > 64 and (hard > 0).sum() > 64
    for op in (0, 3):
        assert set(hard.view(np.uint64).tolist()) <= set(A.args(op)[0].view(np.uint64).tolist())
    x, y = A.args(4)
    assert set((-np.abs(hard)).view(np.uint64).tolist()) <= set(x[y == 0].view(np.uint64).tolist())
    with np.errstate(all="ignore"):
        d = x - y
    for t in A.LOG1PEXP_THRESHOLDS + [-36.04365338911715]:
        assert set(A.around(t).view(np.uint64).tolist()) <= set(d.view(np.uint64).tolist()), t
    pairs = set(zip(x.view(np.uint64).tolist(), y.view(np.uint64).tolist()))
    bits = lambda v: int(np.array([v], np.float64).view(np.uint64)[0])  # noqa: E731
    for a, b in ((np.inf, np.inf), (-np.inf, -np.inf), (np.inf, -np.inf), (1e308, -1e308), (1.25e308, 1.0), (-1.25e308, 1.0), (1.0, 1.0)):
        assert (bits(a), bits(b)) in pairs, (a, b)
    assert (np.isnan(x) & ~np.isnan(y)).any() and (~np.isnan(x) & np.isnan(y)).any() and (d == 0).sum() > 500


@pytest.mark.parametrize("op", [0, 2, 3, 4])
def test_header_matches_host_libm_on_the_shared_arguments(shim, op):
    """the arguments tests/test_gpu_libm.py holds the DEVICE build of the header to the host build on (tests/libm_args.py): here the
    host build against the C library's exp and log1p and the reference's if/else composites over them, bit for bit -- the chain
    device == header == C library on one argument set"""
    from tests import libm_args as A
    x, y = A.args(op)
    ev = A.host_evaluator()
    got, want = ev("header", op, x, y), ev("libm", op, x, y)
    bad = A.differing(got, want)
    assert bad.size == 0, A.report(A.OPS[op], bad, x, y, got, want)
