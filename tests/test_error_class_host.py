"""The class beside the library's error message (include/swd.h, swd_error_class), through the entry points that need no device:
which refusals are SWD_ERR_CAPACITY -- the only class a fallback follows --, which are not, what a later success leaves of them,
and the one place in Python (_lib.error) that turns message and class into an exception.  The last two tests read source text in
the way of tests/test_build_switches.py: nothing branches on the text of a message any more."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import slidingwindowdecoder_amd as S
from slidingwindowdecoder_amd import CapacityError, _lib
from slidingwindowdecoder_amd.decoders import _Csr, _gdg_params, window_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "slidingwindowdecoder_amd")

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libswd_hip.so not built (run __graft_entry__.build())")

WIDE = np.ones((1, 70), np.uint8)                              # row weight 70: beyond every window kernel, fine for the general form
EMPTY_ROW = np.array([[1, 1, 0, 1], [0, 0, 0, 0]], np.uint8)   # no form takes it
SMALL = np.array([[1, 1, 0, 1], [0, 1, 1, 1]], np.uint8)


def _rand(m=20, n=60, seed=3):
    rng = np.random.default_rng(seed)
    H = np.zeros((m, n), np.uint8)
    for c in range(n):
        H[rng.choice(m, 3, replace=False), c] = 1
    H[np.arange(m), np.arange(m)] = 1  # no empty row
    return H


def _forms(H, p=None, gp=None):
    """swd_window_forms on the one window H -> (return code, plan record)"""
    csr = _Csr(H, np.full(H.shape[1], 0.1))
    desc = (_lib.WindowDesc * 1)()
    desc[0].graph = csr.desc
    plan = np.full(_lib.FORM_PLAN_WORDS, -7, np.int32)
    rc = _lib.lib().swd_window_forms(1, C.cast(desc, C.c_void_p), 0, C.byref(p) if p else None, C.byref(gp) if gp else None,
                                     plan.ctypes.data, None)
    return rc, plan


def _osdw(method=0, order=0):
    return _lib.OsdwParams(8, 100, 1.0, 0, method, order)


def test_capacity_error_is_both_a_value_error_and_a_runtime_error():
    assert issubclass(CapacityError, ValueError) and issubclass(CapacityError, RuntimeError)
    assert S.CapacityError is CapacityError and "CapacityError" in S.__all__
    assert (_lib.ERR_FAILED, _lib.ERR_VALUE, _lib.ERR_CAPACITY, _lib.ERR_DEVICE) == (0, 1, 2, 3)  # include/swd.h
    hdr = open(os.path.join(ROOT, "include", "swd.h")).read()
    assert re.search(r"SWD_ERR_FAILED = 0, SWD_ERR_VALUE = 1, SWD_ERR_CAPACITY = 2, SWD_ERR_DEVICE = 3", hdr)


def test_window_forms_reports_the_general_form_for_a_capacity_refusal_only():
    rc, plan = _forms(WIDE, p=_osdw())
    assert rc == 0 and plan[10] == 1
    assert _lib.last_error_class() == _lib.ERR_CAPACITY and "has weight 70 > 64" in _lib.last_error()
    err = _lib.error("swd_window_forms")
    assert type(err) is CapacityError and str(err) == f"swd_window_forms failed: {_lib.last_error()}"
    assert window_forms([(WIDE, np.full(70, 0.1))])["general"] == 1

    # an empty row: input no form takes -- refused, not reported as general = 1
    rc, plan = _forms(EMPTY_ROW, p=_osdw())
    assert rc == -1 and (plan == -7).all()
    assert _lib.last_error_class() not in (_lib.ERR_CAPACITY, _lib.ERR_DEVICE) and "is empty" in _lib.last_error()
    with pytest.raises(ValueError, match="row 1 is empty"):
        window_forms([(EMPTY_ROW, np.full(4, 0.1))])

    # osd_e beyond the device's order: the general form refuses the same, so no capacity matter
    rc, _ = _forms(_rand(), p=_osdw(1, 16))
    assert rc == -1 and _lib.last_error_class() == _lib.ERR_FAILED and "osd_e supports osd_order <= 15" in _lib.last_error()
    assert type(_lib.error("swd_window_forms")) is RuntimeError


def test_value_refusals_become_value_errors_with_the_bare_message():
    rc, _ = _forms(SMALL, p=_osdw(2, 43))  # new_n - rank = 4 - 2
    assert rc == -1 and _lib.last_error_class() == _lib.ERR_VALUE
    msg = "For this code, the OSD order should be set in the range 0<=osd_oder<=2."
    assert _lib.last_error() == msg
    err = _lib.error("swd_window_forms")
    assert type(err) is ValueError and str(err) == msg
    assert str(_lib.error("swd_window_forms", prefix_value=True)) == "swd_window_forms failed: " + msg
    rc, _ = _forms(SMALL, p=_osdw(5, 0))
    assert rc == -1 and _lib.last_error_class() == _lib.ERR_VALUE and "OSD method '5' invalid" in _lib.last_error()
    gp = _gdg_params({}, 0)
    gp.max_tree_depth = 7
    rc, _ = _forms(SMALL, gp=gp)
    assert rc == -1 and _lib.last_error_class() == _lib.ERR_VALUE and "invalid guessing-decoder parameters" in _lib.last_error()


def test_guessing_decoder_size_refusals_are_capacity():
    # max_guess = 2 (2^6 - 1) + 200 - 6 = 320 snapshots, the device keeps 160
    rc, plan = _forms(SMALL, gp=_gdg_params(dict(max_tree_depth=6, max_side_depth=200), 0))
    assert rc == 0 and plan[10] == 1
    assert _lib.last_error_class() == _lib.ERR_CAPACITY and "max_guess=320 exceeds the device limit of 160 snapshots" in _lib.last_error()
    assert window_forms([(SMALL, np.full(4, 0.1))], decoder="bpgdg_decoder", max_tree_depth=6, max_side_depth=200)["general"] == 1
    # the threaded ensemble: at most 158 side threads
    rc, plan = _forms(SMALL, gp=_gdg_params(dict(max_tree_depth=0, max_side_depth=159, multi_thread=True), 0))
    assert rc == 0 and plan[10] == 1 and _lib.last_error_class() == _lib.ERR_CAPACITY and "multi_thread: at most 158" in _lib.last_error()


def test_a_success_leaves_the_last_failure_standing():
    """as swd_last_error() always did: message and class describe the thread's most recent FAILURE"""
    L = _lib.lib()
    v = [C.c_int32(-7) for _ in range(8)]
    assert L.swd_bp4_last_form(None, *[C.byref(x) for x in v]) == -1
    assert _lib.last_error_class() == _lib.ERR_FAILED and _lib.last_error() == "null decoder"
    assert type(_lib.error("swd_bp4_last_form")) is RuntimeError and str(_lib.error("swd_bp4_last_form")) == "swd_bp4_last_form failed: null decoder"
    rc, _ = _forms(WIDE, p=_osdw())
    assert rc == 0 and _lib.last_error_class() == _lib.ERR_CAPACITY
    msg = _lib.last_error()
    rc, plan = _forms(SMALL, p=_osdw())  # succeeds without a refusal on the way
    assert rc == 0 and plan[10] == 0
    assert L.swd_abi_version() == 4
    assert _lib.last_error() == msg and _lib.last_error_class() == _lib.ERR_CAPACITY


def test_front_end_template_refusals_are_neither_capacity_nor_device():
    from slidingwindowdecoder_amd.decoders import _template_desc
    from slidingwindowdecoder_amd.measurements import measurement_map
    from tests.test_measurement_host import case
    L = _lib.lib()
    ops, h, mpr, fin = case("bb72z")
    blk = measurement_map(ops, h).blocks()

    def create(head, body, tail, obs, fin_=fin):
        keep = []
        d = [_template_desc(t, keep) for t in (head, body, tail, obs)]
        return L.swd_frontend_create(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), C.byref(d[3]), mpr, fin_, h, 4, 0)
    for args, kw, text in (((blk.body, blk.body, blk.tail, blk.obs_tail), {}, "head template: row 0 reads column 0 outside [72, 144)"),
                           ((blk.head, blk.tail[:, :2 * mpr], blk.tail[:h - 1], blk.obs_tail), {}, "the tail template is 35 x 144, expected 36 x 144"),
                           ((blk.head, blk.body, blk.tail, blk.obs_tail), dict(fin_=40000), "exceed the 32768 bytes a launch stages")):
        assert not create(*args, **kw)
        assert text in _lib.last_error() and _lib.last_error_class() not in (_lib.ERR_CAPACITY, _lib.ERR_DEVICE)
        assert type(_lib.error("swd_frontend_create")) is RuntimeError


def test_no_device_is_a_device_failure_and_never_a_fallback():
    """what used to be a candidate for the general form: a create that fails because no device is there"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no HIP device") as e:
        S.osd_window(np.eye(4, dtype=np.uint8), channel_probs=np.full(4, 0.1))
    assert not isinstance(e.value, ValueError)
    assert _lib.last_error_class() == _lib.ERR_DEVICE


def test_python_branches_on_no_message_text():
    text = open(os.path.join(PKG, "decoders.py"), encoding="utf-8").read()
    assert "in msg" not in text and "msg.startswith" not in text
    assert "_lib.error(" in text and "last_error_class() == _lib.ERR_CAPACITY" in text


def test_the_library_searches_no_message_text():
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*"))):
        if not path.endswith((".h", ".hip")):
            continue
        text = open(path, encoding="utf-8").read()
        assert not re.search(r"last_error\(\)\s*(?:\.|->)?\s*find\(|str(?:str|n?cmp)\s*\(\s*(?:swd::)?last_error\(\)", text), path
        for name in re.findall(r"(\w+)\s*=\s*(?:swd::)?last_error\(\)", text):  # a copy of the message may be re-raised, never searched
            assert not re.search(r"\b%s\s*\.\s*(?:find|rfind|compare|substr)\(" % re.escape(name), text), f"{os.path.basename(path)}: {name}"
