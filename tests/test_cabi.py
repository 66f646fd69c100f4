"""The C-ABI library loads on a CPU-only host and exports every symbol include/swd.h declares
(no compute calls here: decoding needs the GPU)."""
import os
import re

import pytest

from slidingwindowdecoder_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "swd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(swd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 10
    bound = {s[0] for s in _lib.SYMBOLS}
    for nme in names:
        assert hasattr(L, nme), f"{nme} declared in include/swd.h but not exported"
        assert nme in bound, f"{nme} has no ctypes prototype in _lib.SYMBOLS"
    assert L.swd_abi_version() == 4


def test_no_cpu_fallback():
    """Without a GPU, constructing a decoder must fail loudly (never route to a CPU path)."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built")
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from slidingwindowdecoder_amd import osd_window
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        osd_window(np.eye(4, dtype=np.uint8), channel_probs=np.full(4, 0.1))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "slidingwindowdecoder_amd")
    for dp, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, fn)).read()
                assert "swd_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, fn


def test_bp4_last_form_is_bound_and_refuses_a_null_handle():
    """swd_bp4_last_form (the form of the BP kernel a handle's last launch took) answers without a GPU for a null handle: -1 and
    a message, the out-parameters untouched; the Python surface reads it as ``bp4_osd.last_form``."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built")
    import ctypes as C
    from slidingwindowdecoder_amd import bp4_osd
    L = _lib.lib()
    v = [C.c_int32(-7) for _ in range(8)]
    assert L.swd_bp4_last_form(None, *[C.byref(x) for x in v]) == -1
    assert "null" in _lib.last_error()
    assert all(x.value == -7 for x in v)
    assert L.swd_bp4_last_form(None, *([None] * 8)) == -1
    assert isinstance(bp4_osd.last_form, property)


def test_window_form_reports_are_bound_and_refuse_a_null_handle():
    """swd_osdw_last_form / swd_gdg_last_form / swd_pipeline_last_form answer without a GPU for a null handle: -1 and a message, the
    records untouched; swd_window_forms needs no device at all and refuses a call without windows or with both or neither of the two
    parameter records; the Python surface reads them as ``last_form`` and ``window_forms``."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built")
    import numpy as np
    import slidingwindowdecoder_amd as S
    L = _lib.lib()
    for name in ("swd_osdw_last_form", "swd_gdg_last_form", "swd_pipeline_last_form"):
        plan = np.full(_lib.FORM_PLAN_WORDS, -7, np.int32)
        wins = np.full(_lib.FORM_WINDOW_WORDS, -7, np.int32)
        assert getattr(L, name)(None, plan.ctypes.data, wins.ctypes.data) == -1
        assert "null" in _lib.last_error()
        assert (plan == -7).all() and (wins == -7).all()
        assert getattr(L, name)(None, None, None) == -1
    for cls in (S.osd_window, S.bp_history_decoder, S.bpgdg_decoder, S.bpgd_decoder, S.SlidingWindowDecoder):
        assert isinstance(cls.last_form, property)
    import ctypes as C
    p, gp = _lib.OsdwParams(8, 100, 1.0, 0, 0, 0), S.decoders._gdg_params({}, 0)
    assert L.swd_window_forms(0, None, 0, C.byref(p), None, None, None) == -1
    H = np.array([[1, 1, 0, 1], [0, 1, 1, 1]], np.uint8)
    csr = S.decoders._Csr(H, np.full(4, 0.1))
    desc = (_lib.WindowDesc * 1)()
    desc[0].graph = csr.desc
    plan = np.full(_lib.FORM_PLAN_WORDS, -7, np.int32)
    assert L.swd_window_forms(1, C.cast(desc, C.c_void_p), 0, C.byref(p), C.byref(gp), plan.ctypes.data, None) == -1
    assert L.swd_window_forms(1, C.cast(desc, C.c_void_p), 0, None, None, plan.ctypes.data, None) == -1
    assert (plan == -7).all()
    f = S.window_forms([(H, np.full(4, 0.1))])
    assert (f["nt"], f["vf"], f["dm"], f["kg"], f["general"], f["kind"]) == (64, 4, 4, 2, 0, -1) and len(f["windows"]) == 1
    # a graph no window kernel takes is reported, not refused
    wide = np.ones((1, 70), np.uint8)
    assert S.window_forms([(wide, np.full(70, 0.1))])["general"] == 1
