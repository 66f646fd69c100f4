"""The host policy of the experiments' ``run`` (decoders._run_batches: which shots go to which lane, when the error counter may be
read and the run may stop) and the search for the smallest rolling template (decoders._smallest_rolling_template), with recording
fakes in place of the device."""
import pytest

from slidingwindowdecoder_amd import windows
from slidingwindowdecoder_amd.decoders import _run_batches, _smallest_rolling_template


class Fake:
    """records every call in order; ``errors_after[j]``: what the counter holds once j batches have been enqueued"""

    def __init__(self, errors_after=None):
        self.log, self.errors_after = [], errors_after or {}

    def enqueue(self, lane, B, start):
        self.log.append(("enqueue", lane, B, start))

    def sync(self, lanes):
        self.log.append(("sync", lanes))

    def errors(self):
        self.log.append(("read",))
        return self.errors_after.get(len(self.batches), 0)

    @property
    def batches(self):
        return [e[1:] for e in self.log if e[0] == "enqueue"]

    def run(self, shots, batch, lanes, first_shot=0, max_errors=None):
        return _run_batches(shots, batch, lanes, first_shot, max_errors, self.enqueue, self.sync, self.errors)


@pytest.mark.parametrize("shots, batch, lanes, want", [
    (10, 4, 2, [(0, 4, 0), (1, 4, 4), (0, 2, 8)]),
    (8, 4, 2, [(0, 4, 0), (1, 4, 4)]),
    (5, 7, 3, [(0, 5, 0)]),
    (0, 4, 2, []),
    (0, 1, 5, []),
    (9, 2, 3, [(0, 2, 0), (1, 2, 2), (2, 2, 4), (0, 2, 6), (1, 1, 8)]),
])
def test_batches_are_cut_and_go_round_the_lanes(shots, batch, lanes, want):
    f = Fake()
    assert f.run(shots, batch, lanes) == shots
    assert f.batches == want
    assert f.log == [("enqueue",) + b for b in want]  # no max_errors: no lane is joined inside the loop, the counter is never read
    g = Fake()
    g.run(shots, batch, lanes, first_shot=1000)
    assert g.batches == [(lane, B, start + 1000) for lane, B, start in want]


def test_no_shots_read_no_counter_even_with_max_errors():
    f = Fake({0: 99})
    assert f.run(0, 4, 2, max_errors=1) == 0 and f.log == []


def test_max_errors_stops_after_the_round_of_lanes_is_complete():
    f = Fake({1: 1, 2: 1})  # the first batch already holds the error
    assert f.run(40, 4, 2, max_errors=1) == 8
    assert f.log == [("enqueue", 0, 4, 0), ("enqueue", 1, 4, 4), ("sync", 2), ("read",)]


def test_max_errors_stops_at_the_threshold_not_before():
    f = Fake({2: 1, 4: 2, 6: 3})
    assert f.run(40, 4, 2, max_errors=2) == 16 and len(f.batches) == 4
    g = Fake({2: 5})  # the count may overshoot: >= stops
    assert g.run(40, 4, 2, max_errors=2) == 8
    h = Fake()  # never reached: every round is checked, every shot is run
    assert h.run(40, 4, 2, max_errors=1) == 40 and h.log.count(("read",)) == 5


def test_a_final_partial_round_is_not_checked():
    f = Fake({5: 7})  # errors that show only in the partial round do not matter: nothing reads them
    assert f.run(20, 4, 3, max_errors=1) == 20
    assert len(f.batches) == 5 and f.log.count(("read",)) == 1 and f.log[-2][0] == "enqueue" and f.log[-1][0] == "enqueue"
    assert f.log[:5] == [("enqueue", 0, 4, 0), ("enqueue", 1, 4, 4), ("enqueue", 2, 4, 8), ("sync", 3), ("read",)]


def test_the_counter_is_read_only_after_the_lanes_of_the_round_were_joined():
    f = Fake()
    f.run(64, 4, 4, max_errors=10 ** 9)
    reads = [i for i, e in enumerate(f.log) if e == ("read",)]
    assert len(reads) == 4
    for i in reads:
        assert f.log[i - 1] == ("sync", 4) and [e[0] for e in f.log[i - 5:i - 1]] == ["enqueue"] * 4
    assert f.log.count(("sync", 4)) == len(reads)  # lanes are joined inside the loop for a read alone


# ---- the smallest rolling template ------------------------------------------------------------------------------------------------
def search(monkeypatch, num_repeat, W, F, refuse):
    """-> (result, R0s planned); ``rolling_template`` refuses the plans of the lengths in ``refuse``"""
    tried = []

    def make_plan(R0):
        tried.append(R0)
        return f"plan{R0}", f"extras{R0}"

    def template(plan):
        if int(plan[4:]) in refuse:
            raise ValueError(f"{plan} is not periodic")
    monkeypatch.setattr(windows, "rolling_template", template)
    try:
        return _smallest_rolling_template(num_repeat, W, F, make_plan, "MemoryExperiment.bb"), tried
    except ValueError as e:
        return e, tried


def test_template_search_takes_the_first_length_that_is_accepted(monkeypatch):
    got, tried = search(monkeypatch, 9, 3, 1, refuse=())
    assert got == ("plan3", "extras3") and tried == [3]
    got, tried = search(monkeypatch, 10, 4, 2, refuse={4})  # R0 = 4 (mod 2): 4 is refused, 4 + F is tried and returned
    assert got == ("plan6", "extras6") and tried == [4, 6]
    got, tried = search(monkeypatch, 9, 4, 2, refuse=())  # W + (9 - 4) % 2 = 5: the least R0 >= W with R0 = 9 (mod 2)
    assert got == ("plan5", "extras5") and tried == [5]


def test_template_search_relays_the_last_refusal(monkeypatch):
    err, tried = search(monkeypatch, 7, 3, 2, refuse={3, 5, 7})
    assert isinstance(err, ValueError) and tried == [3, 5, 7]
    assert str(err) == ("no rolling template serves 7 rounds with (W, F) = (3, 2): it needs R0 = 7 (mod 2), R0 <= 7, periodic between "
                        "its first and its last window, and R0 = 7: plan7 is not periodic.  Use MemoryExperiment.bb for an experiment "
                        "this short")


def test_template_search_of_an_experiment_shorter_than_a_window(monkeypatch):
    err, tried = search(monkeypatch, 2, 3, 1, refuse=())
    assert isinstance(err, ValueError) and tried == [] and "and none was tried.  Use MemoryExperiment.bb for" in str(err)
