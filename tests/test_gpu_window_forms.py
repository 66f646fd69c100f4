"""Every case of tests/window_forms.py on the device: the decoder reports the form the host probe promised
(tests/test_window_forms_host.py) and the kernel kind the case is for, and every output equals the oracle's -- decoded vectors, exit
classes, BP iterations, min_pm (float ==), the OSD-0 vectors of the elimination cases; for the guessing decoders the converge
flags and, for the threaded ensemble, the winner, tie count and BP blocks; for pipelines total_e_hat and the per-window records."""
import numpy as np
import pytest

from tests import window_forms as T
from tests.test_window_forms_host import PLAN_FIELDS

pytestmark = pytest.mark.gpu


def assert_last_form(dec, name):
    want = T.expected(name)
    got = dec.last_form
    for k in PLAN_FIELDS + ("kind", "stream_serial", "depth_launch"):
        assert got[k] == want[k], f"{name}: {k}: {got[k]} != {want[k]}"
    assert len(got["windows"]) == len(want["windows"])
    for g, w in zip(got["windows"], want["windows"]):
        assert g == w, f"{name}: {g} != {w}"


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES if c["decoder"] == "osd_window"])
def test_osd_window_case(name):
    from slidingwindowdecoder_amd import osd_window, window_forms
    c = T.case(name)
    H, pr, synd = T.problem(c)
    want, res, osd0 = T.oracle_osdw(name)
    dev = osd_window(H, channel_probs=pr, **c["kw"])
    before = dev.last_form
    assert before["kind"] == -1 and before["windows"] == window_forms([(H, pr)], **c["kw"])["windows"]
    out = dev.decode_batch(synd, return_osd0=c["osd0"])
    assert_last_form(dev, name)
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, f"{name}: shots {bad[:8].tolist()} differ, oracle exits {res['exit_class'][bad[:8]].tolist()}"
    assert np.array_equal(dev.last_status & 0xFF, res["exit_class"])
    assert np.array_equal(dev.last_iterations, res["bp_iteration"])
    assert np.array_equal(dev.last_min_pm, res["min_pm"])
    if c["osd0"]:
        through = res["exit_class"] == 2
        assert np.array_equal(dev.last_osd0[through], osd0[through])


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES if c["decoder"] != "osd_window"])
def test_guessing_decoder_case(name, monkeypatch):
    import slidingwindowdecoder_amd as S
    c = T.case(name)
    for k, v in c["env"].items():  # (read when the decoder is built)
        monkeypatch.setenv(k, v)
    H, pr, synd = T.problem(c)
    want, conv, post, pm, info = T.oracle_gdg(name)
    dev = getattr(S, c["decoder"])(H, channel_probs=pr, **c["kw"])
    out = dev.decode_batch(synd)
    assert_last_form(dev, name)
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, f"{name}: shots {bad[:8].tolist()} differ"
    assert np.array_equal((dev.last_status & 0x100) != 0, conv)
    assert np.array_equal((dev.last_status & 0xFF) != 0, post)
    if info is not None:  # the threaded ensemble: path metric, winner, ties and BP blocks of every shot whose ensemble ran
        ran = post & ((dev.last_status & 0xFF) != 4)
        assert np.array_equal(dev.last_min_pm[ran], pm[ran])
        assert np.array_equal(dev.last_stats[ran][:, [6, 7, 5]], info[ran])


@pytest.mark.parametrize("name", list(T.PIPELINES))
def test_pipeline_case(name):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from tests.test_gpu_node_depth import check_pipeline, oracle_pipeline
    p = T.PIPELINES[name]
    plan, det = T.pipeline_problem(name)
    want, cls, its, pm = oracle_pipeline(plan, np.array(det), p["kw"])
    assert (cls == 2).sum() >= 4
    dec = SlidingWindowDecoder(plan, **p["kw"])
    check_pipeline(dec, det, want, cls, its, pm, name)
    assert_last_form(dec, name)
