#!/usr/bin/env python3
"""Randomised bp4_osd device-vs-oracle comparison (run by hand or from the GPU suite):
    python tests/fuzz_bp4.py [trials] [seed] [min qubits] [max qubits]
Random ragged Hx / Hz, X/Y/Z priors, iteration counts, scaling factors and OSD methods.  The device evaluates
exp / log1p like glibc's FMA build (csrc/swd_libm.h); on a host whose libm selects that build (x86-64 with FMA,
glibc >= 2.28) the oracle and the device must agree on EVERY shot -- vector, converge flag, iteration count, BP decisions -- and
every posterior LLR bit for bit, non-finite posteriors included (NaN at the same positions); only the vector of an unconverged shot
whose OSD ordering keys contain a NaN is not compared (the reference's std::stable_sort leaves that order undefined).  On any
other host the oracle's own libm differs in the last bit: there up to 2 % of a trial's shots may differ and the
LLRs are held to 1e-5 (1e-2 beyond 10 iterations, where non-converging BP amplifies a last-bit difference).

    --form NAME   demand one form of the BP kernel (FORMS below): its SWD_BP4_* switches are set (and every other SWD_BP4_*
                  switch cleared) before the library reads them, n is drawn from the form's range unless given, and a trial
                  whose launch reports another form (bp4_osd.last_form) fails.  The switches are read once per process.
    --skew P      SWD_BP4_SKEW=P (even / odd): the waves of that parity sleep before every message-storing node pass of a
                  split launch (csrc/swd_bp4_kernel.h bp4_skew); the form must report it.
    --prefix      adversarial codes for the unequal-rank OSD shortcut: rank(Hx) > rank(Hz), and the first kx + rank_z columns
                  of the z-basis order span less than rank_z (tests/golden/make_golden.py gen_bp4_unequal_prefix).
    --trials / --seed / --nmin / --nmax   the positional arguments, by name."""
import argparse
import os
import sys

import numpy as np

# form name: (switches, qubit range [lo, hi), what bp4_osd.last_form must report).  split: two threads per qubit while 2 n <= 256
# (SWD_BP4_SPLIT_MAX raises the bound); the pair of a qubit spans two waves from n > 32 on.
FORMS = {
    "split": ({}, (24, 129), dict(split=1, lazy=0, fast=1, wmax=4)),
    "split_lazy": ({"SWD_BP4_OVERLAPPED": "1"}, (24, 129), dict(split=1, lazy=1, fast=1, wmax=4, overlapped=1)),
    "split8": ({"SWD_BP4_SPLIT_MAX": "512"}, (129, 257), dict(split=1, lazy=1, fast=1, wmax=8)),
    "nosplit_lazy": ({"SWD_BP4_NOSPLIT": "1"}, (12, 400), dict(split=0, lazy=1, fast=1)),
    "nosplit_fused": ({"SWD_BP4_NOSPLIT": "1", "SWD_BP4_NO_LAZY": "1"}, (12, 400), dict(split=0, lazy=0, fast=1)),
    "generic": ({"SWD_BP4_GENERIC": "1"}, (12, 400), dict(split=0, lazy=0, fast=0)),
}

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("pos", nargs="*", type=int, help="[trials] [seed] [min qubits] [max qubits]")
ap.add_argument("--trials", type=int)
ap.add_argument("--seed", type=int)
ap.add_argument("--nmin", type=int)
ap.add_argument("--nmax", type=int)
ap.add_argument("--form", choices=sorted(FORMS))
ap.add_argument("--skew", choices=["even", "odd"])
ap.add_argument("--prefix", action="store_true")
args = ap.parse_args()
pos = list(args.pos) + [None] * 4
want_form = None
if args.form or args.skew:
    for k in [k for k in os.environ if k.startswith("SWD_BP4_")]:
        del os.environ[k]
    env, rng_n, want_form = FORMS[args.form] if args.form else ({}, (None, None), {})
    want_form = dict(want_form)
    os.environ.update(env)
    if args.skew:
        os.environ["SWD_BP4_SKEW"] = args.skew
        want_form["skew"] = 1 if args.skew == "even" else 2
    if not args.prefix:  # (the adversarial codes have a range of their own, inside the split forms' range)
        pos[2] = pos[2] if pos[2] is not None else rng_n[0]
        pos[3] = pos[3] if pos[3] is not None else rng_n[1]

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
from slidingwindowdecoder_amd import bp4_osd  # noqa: E402
from tests.test_oracle_bp4 import z_prefix_deficient  # noqa: E402
from tests.test_oracle_bp4_nonfinite import keys_have_nan  # noqa: E402

def _host_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def _pick(named, p, default):
    return named if named is not None else (p if p is not None else default)


EXACT = _host_fma()
trials = _pick(args.trials, pos[0], 30)
rng = np.random.default_rng(_pick(args.seed, pos[1], 1))
NMIN, NMAX = _pick(args.nmin, pos[2], 30 if args.prefix else 12), _pick(args.nmax, pos[3], 53 if args.prefix else 400)  # qubits: the BP kernel runs on ceil(n / 64) waves up to 1024 threads


def rand_h(m, n):
    H = (rng.random((m, n)) < rng.uniform(1.5, 3.0) / m).astype(np.uint8)
    for r in range(m):
        if H[r].sum() == 0:
            H[r, rng.integers(n)] = 1
    for c in range(n):
        if H[:, c].sum() == 0:
            H[rng.integers(m), c] = 1
    return H


def prefix_case(n):
    """rank(Hx) > rank(Hz) where the unequal-rank shortcut is weakest: Hx of full row rank n - kx (kx small); outside a set S
    every Hz column is the same single check (rank 1 together), Hz's other rank lies on S, and S has priors far below the
    rest, so S sorts last in the z basis and the first kx + rank_z sorted columns span less than rank_z."""
    kx = int(rng.integers(3, 7))
    mx, ns = n - kx, int(rng.integers(max(8, n - 38), max(9, n // 2)))
    S = rng.choice(n, size=ns, replace=False)
    Hx = np.zeros((mx, n), np.uint8)
    piv = rng.permutation(n)
    for i in range(mx):  # upper-triangular over the pivot columns: full row rank
        Hx[i, piv[i]] = 1
        if i > 0:
            Hx[rng.choice(i, size=min(i, int(rng.integers(0, 3))), replace=False), piv[i]] = 1
    for c in piv[mx:]:
        Hx[rng.choice(mx, size=3, replace=False), c] = 1
    mz = int(rng.integers(5, ns - 2))
    Hz = np.zeros((mz, n), np.uint8)
    Hz[0, :] = 1
    Hz[:, S] = 0
    for j, c in enumerate(S):
        rows = rng.choice(np.arange(1, mz), size=int(rng.integers(2, 4)), replace=False)
        Hz[rows, c] = 1
        Hz[1 + j % (mz - 1), c] = 1  # every check of Hz is used
    lo = np.ones(n, bool)
    lo[S] = False
    pr = [np.where(lo, rng.uniform(0.01, 0.05, size=n), rng.uniform(1e-5, 1e-4, size=n)) for _ in range(3)]
    return Hx, Hz, pr, kx


bad = done = 0
prefix_hits = 0
while done < trials:
    n = int(rng.integers(NMIN, NMAX))
    if args.prefix:
        Hx, Hz, pr, kx = prefix_case(n)
    else:
        mx, mz = int(rng.integers(4, max(5, n // 2))), int(rng.integers(4, max(5, n // 2)))
        Hx, Hz = rand_h(mx, n), rand_h(mz, n)
    mx, mz = Hx.shape[0], Hz.shape[0]
    if max(Hx.sum(0).max(), Hz.sum(0).max()) > 8 or max(Hx.sum(1).max(), Hz.sum(1).max()) > 40 or (Hx.sum(0) == 0).any() or (Hz.sum(0) == 0).any():
        continue
    if not args.prefix:
        pr = [rng.uniform(0.001, 0.03, size=n) for _ in range(3)]
    method = ["osd_cs", "osd_e"][int(rng.integers(2))] if args.prefix else ["osd_0", "osd_cs", "osd_e"][int(rng.integers(3))]
    kw = dict(channel_probs_x=pr[0], channel_probs_y=pr[1], channel_probs_z=pr[2], max_iter=int(rng.integers(1, 7 if args.prefix else 40)),
              ms_scaling_factor=float(rng.choice([1.0, 0.9, 0.75, 0.625])), osd_method=method,
              osd_order=int(rng.integers(1, kx + 1)) if args.prefix else (0 if method == "osd_0" else int(rng.integers(0, 5))))
    try:
        ora = O.bp4_osd(Hx, Hz, **kw)
    except ValueError:
        continue
    try:
        dev = bp4_osd(Hx, Hz, **kw)
    except (ValueError, RuntimeError) as ex:
        if "rank(Hx) < rank(Hz)" in str(ex):
            continue  # documented: the reference reads past its column array there (rank(Hx) > rank(Hz) is decoded, and compared)
        print(f"trial {done}: device rejected n={n} mx={mx} mz={mz}: {ex}")
        bad += 1; done += 1
        continue
    done += 1
    B = 100
    u = rng.random((B, n))
    sc = rng.uniform(0.5, 3.0)
    ex = (u < sc * (pr[0] + pr[1])).astype(np.uint8)                        # X or Y component
    ez = ((u >= sc * pr[0]) & (u < sc * (pr[0] + pr[1] + pr[2]))).astype(np.uint8)  # Y or Z component
    sx, sz = (ez @ Hx.T) % 2, (ex @ Hz.T) % 2
    out = dev.decode_batch(sx, sz)
    form = dev.last_form
    if want_form and any(form.get(k) != v for k, v in want_form.items()):
        print(f"trial {done}: FORM MISMATCH n={n}: demanded {want_form}, the launch took {form}")
        bad += 1
        continue
    if args.prefix:
        assert dev.rank_x > dev.rank_z and dev.rank_x == Hx.shape[0]
    diff = llr_bad = 0
    worst = 0.0
    for b in range(B):
        w = ora.decode(sx[b], sz[b])
        if args.prefix and not ora.converge and np.isfinite(ora.log_prob_ratios).all():
            prefix_hits += z_prefix_deficient(ora.log_prob_ratios, Hz, Hx.shape[1] - dev.rank_x, dev.rank_z)
        lpr_o = ora.log_prob_ratios
        # a qubit under several degree-1 checks collects +-1e308 sentinels: inf / NaN posteriors.  BP itself is defined there and
        # compared on EVERY shot -- converge flag, iterations, BP decisions, posteriors with NaN at the same positions (NaN-faithful
        # clip, minimum and sign count) -- and so is the OSD while its ordering keys are NaN-free (infinite keys sort well).  A NaN
        # key goes through std::stable_sort in the reference (bpgd.cpp:384-389), which leaves the order undefined: the vector of
        # such a shot is the one thing not compared (tests/test_gpu_bp4_nonfinite.py pins the same rule on recorded shots)
        vec_ok = np.array_equal(w, out[b]) or (not ora.converge and not np.isfinite(lpr_o).all() and keys_have_nan(lpr_o))
        bp_ok = np.array_equal(np.stack([ora.bp_decoding_x, ora.bp_decoding_z]), dev.last_bp_decoding[b])
        same = vec_ok and bp_ok and bool(ora.converge) == bool(dev.last_status[b] & 0x100) and ora.bp_iteration == dev.last_iterations[b]
        if not same:
            diff += 1
            if os.environ.get("SWD_FUZZ_VERBOSE"):
                a, r = dev.last_llr[b].T, lpr_o
                print(f"   shot {b}: vec differs {int((w != out[b]).sum())} bp decisions {'same' if bp_ok else 'differ'} conv dev {bool(dev.last_status[b] & 0x100)} ora {bool(ora.converge)} its dev "
                      f"{dev.last_iterations[b]} ora {ora.bp_iteration} nonfinite dev {int((~np.isfinite(a)).sum())} ora {int((~np.isfinite(r)).sum())} "
                      f"max|llr| ora {np.nanmax(np.abs(r)):.3g} max abs diff {np.nanmax(np.abs(a - r)):.3g}")
        if EXACT:  # the posteriors of every shot, bit for bit up to the payload of a NaN
            if not np.array_equal(dev.last_llr[b].T, lpr_o, equal_nan=True):
                llr_bad += 1
                with np.errstate(all="ignore"):
                    worst = max(worst, float(np.nanmax(np.abs(dev.last_llr[b].T - lpr_o) / (np.abs(lpr_o) + 1e-3), initial=0.0)))
        elif same and not np.allclose(dev.last_llr[b].T, lpr_o, rtol=1e-5 if kw['max_iter'] <= 10 else 1e-2, atol=1e-8, equal_nan=True):
            llr_bad += 1
            a, r = dev.last_llr[b].T, lpr_o
            worst = max(worst, float(np.max(np.abs(a - r) / (np.abs(r) + 1e-3))))
    # camel_decode (bp4_osd.pyx:223-247) on the first shots, oracle state fresh per shot like the device's
    cam = dev.camel_decode_batch(sx[:24], sz[:24])
    cdiff = 0
    for b in range(24):
        o = O.bp4_osd(Hx, Hz, **kw)
        w = o.camel_decode(sx[b], sz[b])
        okc = np.array_equal(w, cam[b]) and bool(o.converge) == bool(dev.last_status[b] & 0x100)
        if okc and o.converge:
            okc = abs(o.min_pm - dev.last_min_pm[b]) <= 1e-9 * abs(o.min_pm)
        cdiff += not okc
    if cdiff > (0 if EXACT else 1):
        bad += 1
        print(f"trial {done}: camel_decode MISMATCH n={n} mx={mx} mz={mz} differing shots {cdiff}/24 kw={ {k: v for k, v in kw.items() if not k.startswith('channel')} }")
        continue
    if diff > (0 if EXACT else 0.02 * B) or llr_bad:
        bad += 1
        print(f"trial {done}: MISMATCH n={n} mx={mx} mz={mz} differing shots {diff}/{B} llr {llr_bad} worst rel {worst:.2e} kw={ {k: v for k, v in kw.items() if not k.startswith('channel')} }")
print(f"{trials} trials, {bad} mismatching ({'every shot and LLR bit for bit' if EXACT else 'host libm without the FMA exp: tolerances applied'})"
      + (f"; form {want_form}" if want_form else "") + (f"; OSD shots with a rank-deficient z prefix {prefix_hits}" if args.prefix else ""))
if args.prefix and not prefix_hits:
    print("no OSD shot reached a rank-deficient z prefix: the adversarial codes are vacuous")
    bad += 1
sys.exit(1 if bad else 0)
