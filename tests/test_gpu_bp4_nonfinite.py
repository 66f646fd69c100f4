"""bp4_osd on the device where the posteriors are NOT finite (+-inf from the summed +-1e308 sentinels of a qubit under several
degree-1 checks, NaN from inf - inf), against the run recorded from the reference extension (tests/golden/bp4_nonfinite.npz,
tests/test_oracle_bp4_nonfinite.py holds the oracle to the same recording).  On EVERY shot: posteriors bit for bit with NaN at the
same positions, converge flag, iteration count, BP decisions.  On every shot whose OSD ordering keys are NaN-free also the returned
vector and the OSD-0 vectors; a shot with a NaN key goes through std::stable_sort in the reference, which leaves its order
undefined: the vector and the OSD-0 vectors of such a shot are the ONLY things not compared.  Each case is built for one kernel -- the
split form of the tuned BP kernel, its HEAVY instantiation, the general form, the general elimination behind either -- and the test
asserts that the launch took it; the other forms of the tuned kernel are demanded through their switches in a child process."""
import sys

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_bp4 import _bp4_env, _run_child
from tests.test_oracle_bp4_nonfinite import LPR_FULL, SHOTS, TAGS, canonical, load_nonfinite

pytestmark = pytest.mark.gpu
GENERAL_FORM = dict(split=0, lazy=0, fast=0, wmax=0, dm=0, threads=1024, skew=0, overlapped=0)
# the recorded cases under the device kwargs they were built for, and the n70 / osd_cs recording once more with the general BP form
# in front of the general elimination (the reference's run does not depend on the device's form)
CELLS = [(t, None) for t in TAGS] + [("n70_cs3", dict(general_form=True, general_osd=True))]
# the forms of bp4_kernel a graph without heavy columns can take besides the default (tests/fuzz_bp4.py FORMS): switches, last_form
FORMS = {
    "split_lazy": ({"SWD_BP4_OVERLAPPED": "1"}, dict(split=1, lazy=1, fast=1)),
    "nosplit_lazy": ({"SWD_BP4_NOSPLIT": "1"}, dict(split=0, lazy=1, fast=1)),
    "nosplit_fused": ({"SWD_BP4_NOSPLIT": "1", "SWD_BP4_NO_LAZY": "1"}, dict(split=0, lazy=0, fast=1)),
    "generic": ({"SWD_BP4_GENERIC": "1"}, dict(split=0, lazy=0, fast=0)),
}


def _check_form(dec, c, dev_kw, want):
    from slidingwindowdecoder_amd import _lib
    f = dec.last_form
    general = bool(dev_kw.get("general_form", False))
    assert _lib.lib().swd_bp4_is_general(dec._h) == int(general) and dec.general_form is general
    assert dec.general_osd is bool(dev_kw.get("general_osd", False))
    if general:
        assert f == GENERAL_FORM and dec.heavy_columns == (0, 0)
    elif c["n"] == 71:  # the HEAVY instantiation: the generic form with the side list of the one column that touches 20 checks
        assert dec.heavy_columns == (1, 20) and (f["split"], f["lazy"], f["fast"], f["dm"], f["threads"]) == (0, 0, 0, 10, 128)
    elif want is None:  # two threads per qubit (2 n <= 256)
        assert dec.heavy_columns == (0, 0) and (f["split"], f["lazy"], f["fast"], f["threads"]) == (1, 0, 1, (2 * c["n"] + 63) // 64 * 64)
    else:
        assert dec.heavy_columns == (0, 0) and all(f[k] == v for k, v in want.items()), f"demanded {want}, the launch took {f}"


def _check_case(tag, dev_kw=None, want=None):
    from slidingwindowdecoder_amd import bp4_osd
    c = load_nonfinite(tag)
    dev_kw = c["dev_kw"] if dev_kw is None else dev_kw
    dec = bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["kw"], **dev_kw)
    out = dec.decode_batch(c["sx"], c["sz"])
    _check_form(dec, c, dev_kw, want)
    lpr = np.ascontiguousarray(np.transpose(dec.last_llr, (0, 2, 1)))  # [B, n, 3] like log_prob_ratios
    bad = [k for k in range(SHOTS) if fx.h64(canonical(lpr[k])) != c["lpr_hash"][k]]
    full = [k for k in range(LPR_FULL) if canonical(lpr[k]).tobytes() != canonical(c["lpr"][k]).tobytes()]
    if bad or full:
        k = (full or bad)[0]
        where = np.argwhere(canonical(lpr[k]).view(np.uint64) != canonical(c["lpr"][k]).view(np.uint64)) if k < LPR_FULL else []
        print(f"{tag}: posteriors differ on shots {bad} (hash) / {full} (full); shot {k}: " +
              "; ".join(f"qubit {q} component {j}: {float(lpr[k][q, j]).hex()} expected {float(c['lpr'][k][q, j]).hex()}" for q, j in where[:6]))
    assert not bad and not full, f"posteriors differ on shots {sorted(set(bad + full))[:10]}"
    assert np.array_equal(np.isnan(lpr).any(axis=(1, 2)), c["nan_lpr"] != 0)
    assert np.array_equal((dec.last_status & 0x100) != 0, c["converge"] != 0)
    assert np.array_equal(dec.last_iterations, c["its"])
    assert np.array_equal(dec.last_bp_decoding, c["bp_dec"]), "BP decisions"
    defined = c["key_nan"] == 0
    assert (defined & (c["converge"] == 0)).sum() >= 24  # (the fixture's conditions in full: tests/test_oracle_bp4_nonfinite.py)
    assert np.array_equal(out[defined], c["out"][defined]), f"vectors of shots {np.flatnonzero((out != c['out']).any(axis=(1, 2)) & defined)[:10]}"
    assert np.array_equal(dec.last_osd0[defined], c["osd0"][defined]), "OSD-0 vectors"


@pytest.mark.parametrize("tag,dev_kw", CELLS, ids=[t + ("-both" if k else "") for t, k in CELLS])
def test_device_equals_the_reference_on_every_shot(tag, dev_kw):
    _check_case(tag, dev_kw)


def _form_cases(form):
    """(run in a child process with the form's switches: the library reads them once per process)"""
    for tag in ("n24_osd0", "n24_cs3", "n70_osd0", "n70_cs3"):
        _check_case(tag, want=FORMS[form][1])
    print(f"non-finite cases ok on form {form}")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_other_forms_of_the_bp_kernel(form):
    """the n24 / n70 recordings on each of the other forms of bp4_kernel (their check passes and node updates are separate code)"""
    code = f"from tests.test_gpu_bp4_nonfinite import _form_cases; _form_cases({form!r})"
    r = _run_child([sys.executable, "-c", code], _bp4_env(**FORMS[form][0]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"non-finite cases ok on form {form}" in r.stdout
