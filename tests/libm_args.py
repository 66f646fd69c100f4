"""Arguments for the bit-for-bit checks of csrc/swd_libm.h and of the two composites on top of it: one deterministic set per op of
swd_diag_libm (include/swd.h), used by tests/test_gpu_libm.py (device build against host build of the header) and by
tests/test_libm_restatement.py (host build against the C library), so that the chain device == header == C library holds on the
SAME arguments.  At most 2^18 per op.  Per function:

  * the six random classes of tests/csrc/libm_check.c (drawn here with numpy, not with its splitmix64);
  * the special values tests/csrc/libm_check.c lists;
  * around every branch threshold t of the code, the 129 doubles from 64 ulps below t to 64 ulps above it, and their negatives;
  * for exp and everything on top of it, the hard cases of tests/golden/exp_hard_cases.txt: arguments whose value before the last
    rounding lies so close to a rounding boundary that one ulp of the polynomial's coefficient C2 changes the result (about one
    random argument in a million is such a case; tests/golden/make_exp_hard_cases.py finds them).

Thresholds (csrc/swd_libm.h, csrc/swd_bp4_kernel.h):
  exp       2^-54 (1 + x), 512 (careful scale), 1024 (overflow / underflow exits), 709.78.. (largest finite result), -708.39..
            (first subnormal result), -745.13.. (last non-zero result)
  log1p     sqrt(2) - 1 and 1 - 1/sqrt(2) (the two hx cuts of the k = 0 range), 2^-29 and 2^-54 (short forms), 2^53 (u = x), -1,
            2^k sqrt(2) - 1 (the hu < 0x6a09e cut), 2^k - 1 (hu == 0 with f == 0 and with |f| tiny), 2^k (1 + 2^-20) - 1 (the upper
            end of hu == 0)
  log1pexp  36.04365338911715 = -log(DBL_EPSILON) (the case cut), +-50 (the clip of the messages)
  logaddexp pairs with x - y at each log1pexp threshold and at 0, x == y, the infinities, the +-1e308 sentinels of the check pass and
            their sums, NaN in either slot
"""
import numpy as np

MAX_ARGS = 1 << 18
N_CLASS = 36000  # per random class; six classes per function
OPS = {0: "exp", 1: "exp", 2: "log1p", 3: "log1pexp", 4: "logaddexp", 5: "log1pexp", 6: "logaddexp"}

EXP_SPECIAL = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e308, -1e308, 709.782712893384, -745.2, 2.0 ** -60, 512.0, -512.0, 1023.9,
               -1023.9]
LOG1P_SPECIAL = [0.0, -0.0, -1.0, -2.0, np.inf, np.nan, 1e308, 2.0 ** -60, 2.0 ** -30, 2.0 ** 53, 2.0 ** 52, -0.2929, 0.41422, 1.0]
EXP_THRESHOLDS = [2.0 ** -54, 512.0, 1024.0, 709.782712893384, -708.3964185322641, -745.1332191019412]
LOG1P_THRESHOLDS = ([np.sqrt(2.0) - 1.0, 1.0 - 1.0 / np.sqrt(2.0), 2.0 ** -29, 2.0 ** -54, 2.0 ** 53, -1.0]
                    + [2.0 ** k * np.sqrt(2.0) - 1.0 for k in range(4)] + [2.0 ** k - 1.0 for k in range(1, 11)]
                    + [2.0 ** k * (1.0 + 2.0 ** -20) - 1.0 for k in range(11)])
LOG1PEXP_THRESHOLDS = [36.04365338911715, 50.0, -50.0]


def exp_hard_cases():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exp_hard_cases.txt")
    return np.array([float.fromhex(ln) for ln in open(path).read().split("\n") if ln and not ln.startswith("#")])


def around(t, ulps=64):
    """the 2 * ulps + 1 doubles from ``ulps`` below t to ``ulps`` above it (t finite, non-zero, |t| well above the subnormals)"""
    bits = np.array([t], np.float64).view(np.int64)[0]
    return (bits + np.arange(-ulps, ulps + 1, dtype=np.int64)).view(np.float64)


def _with_negatives(thresholds):
    a = np.concatenate([around(t) for t in thresholds])
    return np.concatenate([a, -a])


def _exp_random(rng, n):
    u = lambda: rng.random(n)  # noqa: E731
    return [(u() - 0.5) * 100.0, (u() - 0.5) * 2.0, -u() * 760.0, u() * 712.0, (u() - 0.5) * 1e-3, (u() - 0.5) * np.exp((u() - 0.5) * 100.0)]


def _log1p_random(rng, n):
    u = lambda: rng.random(n)  # noqa: E731
    return [u() * 2.0 - 0.999, np.exp((u() - 0.5) * 1400.0), -np.exp(-u() * 700.0), (u() - 0.5) * 1e-6, np.exp((u() - 0.5) * 80.0), u() * 100.0]


def exp_args():
    rng = np.random.default_rng(0x5EED0)
    return np.concatenate(_exp_random(rng, N_CLASS) + [np.array(EXP_SPECIAL), _with_negatives(EXP_THRESHOLDS), exp_hard_cases()])


def log1p_args():
    rng = np.random.default_rng(0x5EED2)
    return np.concatenate(_log1p_random(rng, N_CLASS) + [np.array(LOG1P_SPECIAL), _with_negatives(LOG1P_THRESHOLDS)])


def log1pexp_args():
    """exp's classes and thresholds (log1pexp's argument is exp's, up to the sign) with its own thresholds, and the values a node
    update can hand it: the sentinels of the check pass and their sums"""
    rng = np.random.default_rng(0x5EED3)
    extra = np.array([1.25e308, -1.25e308, 0.625e308, -0.625e308, 1.7e308, -1.7e308])
    return np.concatenate(_exp_random(rng, N_CLASS) + [np.array(EXP_SPECIAL), extra, _with_negatives(EXP_THRESHOLDS + LOG1PEXP_THRESHOLDS), exp_hard_cases(),
                                                         -exp_hard_cases()])


def logaddexp_args():
    rng = np.random.default_rng(0x5EED4)
    n = N_CLASS
    u = lambda: rng.random(n)  # noqa: E731
    # six random classes: both free; close together; far apart in either order; one huge; tiny differences
    y0 = (u() - 0.5) * 120.0
    xs = [(u() - 0.5) * 120.0, y0 + (u() - 0.5) * 2.0, y0 + 30.0 + u() * 30.0, y0 - 30.0 - u() * 30.0, (u() - 0.5) * 2e308,
          y0 + (u() - 0.5) * 1e-6]
    ys = [(u() - 0.5) * 120.0, y0, y0, y0, (u() - 0.5) * 120.0, y0]
    # x - y at each threshold of log1pexp (either sign: the argument of log1pexp is -|x - y|) and at 0, exactly (y = 0) and after
    # the rounding of a sum (other y)
    d = np.concatenate([_with_negatives(LOG1PEXP_THRESHOLDS), np.array([0.0, -0.0]), np.concatenate([around(2.0 ** -1000), -around(2.0 ** -1000)])])
    for y in (0.0, 1.5, -20.25, 100.0, -1e3, 3e300):
        xs.append(y + d); ys.append(np.full(d.size, y))
        xs.append(np.full(d.size, y)); ys.append(y + d)
    # exp's hard cases: logaddexp evaluates exp(-|x - y|)
    h = -np.abs(exp_hard_cases())
    for y in (0.0, 0.5, -8.0):
        xs += [y + h, np.full(h.size, y)]; ys += [np.full(h.size, y), y + h]
    eq = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 50.0, -50.0, 1e308, -1e308, 1.25e308, -1.25e308, 2.0 ** -1074, np.inf, -np.inf]),
                         (rng.random(512) - 0.5) * 200.0])
    xs.append(eq); ys.append(eq.copy())
    fin = np.array([0.0, -0.0, 1.0, -1.0, 36.04365338911715, 50.0, -50.0, 700.0, -700.0, 1e300, -1e300, 1e308, -1e308, 0.625e308, -0.625e308])
    big = np.array([np.inf, -np.inf, np.nan, 1e308, -1e308, 1.25e308, -1.25e308, 1.7e308, -1.7e308])
    a, b = np.meshgrid(big, np.concatenate([fin, big]))
    xs += [a.ravel(), b.ravel()]; ys += [b.ravel(), a.ravel()]
    return np.concatenate(xs), np.concatenate(ys)


def args(op):
    """(x, y) float64 arrays of equal length for op 0..6 of swd_diag_libm; y is None for the one-argument ops"""
    kind = OPS[op]
    if kind == "logaddexp":
        x, y = logaddexp_args()
    else:
        x, y = {"exp": exp_args, "log1p": log1p_args, "log1pexp": log1pexp_args}[kind](), None
    x = np.ascontiguousarray(x, np.float64)
    assert x.size <= MAX_ARGS and (y is None or y.shape == x.shape)
    return x, (None if y is None else np.ascontiguousarray(y, np.float64))


def differing(got, want):
    """indices where two float64 arrays differ: by bits (so +0.0 != -0.0), except that two NaNs are equal whatever their payload"""
    g, w = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    return np.flatnonzero((g.view(np.uint64) != w.view(np.uint64)) & ~(np.isnan(g) & np.isnan(w)))


def report(name, idx, x, y, got, want):
    """failure text: how many arguments differ and the first one, as hex"""
    i = int(idx[0])
    arg = float(x[i]).hex() + ("" if y is None else ", " + float(y[i]).hex())
    return f"{name}: {idx.size} of {x.size} arguments differ, first #{i}: f({arg}) = {float(got[i]).hex()}, expected {float(want[i]).hex()}"


_EVAL = None


def host_evaluator():
    """tests/csrc/libm_check.c built with gcc -ffp-contract=off (once per process): ``ev(name, op, x, y)`` with name "header" -- the
    host build of csrc/swd_libm.h under the reference's branching composites, right on any CPU: gcc's __builtin_fma is exact with or
    without an FMA unit -- or "libm", the C library's exp / log1p under the same composites"""
    global _EVAL
    if _EVAL is None:
        import ctypes as C
        import os
        import subprocess
        import tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        so = os.path.join(tempfile.mkdtemp(prefix="swd_libm_eval_"), "libm_check.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(root, "slidingwindowdecoder_amd", "csrc"),
                               os.path.join(root, "tests", "csrc", "libm_check.c"), "-o", so, "-lm"])
        L = C.CDLL(so)
        for f in (L.swd_eval_header, L.swd_eval_libm):
            f.restype = C.c_int
            f.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]

        def ev(name, op, x, y=None):
            out = np.empty_like(x)
            rc = getattr(L, "swd_eval_" + name)(op, x.size, x.ctypes.data, None if y is None else y.ctypes.data, out.ctypes.data)
            assert rc == 0
            return out
        _EVAL = ev
    return _EVAL
