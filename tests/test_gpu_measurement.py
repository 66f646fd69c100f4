"""Measurement sessions: the device front end (``MeasurementFrontEnd``, C ABI swd_frontend_*) that turns raw measurement records into
detector rows, alone and in front of the online and the rolling session.  Expected values come from the dense host statement
``detectors_from_measurements_host``, from the sessions fed with detector rows, and from ``decode`` -- never from the front end.
All comparisons are exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, SHOTS = 13, 96


@functools.lru_cache(maxsize=None)
def record_case(tag):
    """(map, rows per round, measurements per round, a random record [96, num_meas], its detectors, its raw observable masks)"""
    from slidingwindowdecoder_amd import measurements as ms
    from slidingwindowdecoder_amd.circuit import bb_memory_ops
    from slidingwindowdecoder_amd.codes import bb_code, rep_code
    from slidingwindowdecoder_amd.shyps import shyps_memory_ops
    if tag == "bb72":  # 72 measurements per round: whole bytes
        code, A, B = bb_code(72)
        mm = ms.measurement_map(bb_memory_ops(code, A, B, 0.004, 6), 36)
    elif tag == "shyps":  # 98 per round: 12.25 bytes
        mm = ms.measurement_map(shyps_memory_ops(3, 0.002, 4), 21)
    else:  # 4 per round: several rounds in a byte
        mm = ms.phenomenological_measurement_map(rep_code(5), np.ones((1, 5), np.uint8), 5)
    blk = mm.blocks()
    assert blk.meas_per_round == {"bb72": 72, "shyps": 98, "rep5": 4}[tag]
    meas = np.random.default_rng(SEED).integers(0, 2, (SHOTS, mm.num_meas)).astype(np.uint8)
    det, obs = ms.detectors_from_measurements_host(mm, meas)
    raw = ms.observable_masks(obs)
    assert det.any() and raw.any()
    for a in (meas, det, raw):
        a.setflags(write=False)
    return mm, blk.n_half, blk.meas_per_round, meas, det, raw


def bit_chunkings(total, mpr):
    """piece sizes over ``total`` bits of syndrome rounds: everything at once; one bit at a time through the first two rounds, then
    the rest; pieces of 7, 13 and 101 bits; round-aligned pieces; empty pieces in between"""
    def fill(sizes):
        out, left = [], total
        for k in sizes:
            out.append(min(k, left))
            left -= out[-1]
        return out + ([left] if left else [])
    cyc = [7, 13, 101] * (total // 121 + 1)
    return {"whole": [total], "bitwise": fill([1] * min(2 * mpr, total)), "odd": fill(cyc), "rounds": fill([mpr] * (total // mpr)),
            "empties": fill([0, mpr + 3, 0, 0, 2 * mpr - 3, 0])}


def as_chunk(bits, packed):
    """[B, k] bits -> (array to hand over, ``packed`` argument)"""
    if not packed:
        return np.ascontiguousarray(bits), False
    return np.packbits(bits, axis=1, bitorder="little"), int(bits.shape[1])  # a chunk may end inside a byte: the bit count goes along


def feed(push, finish, meas, sizes, synd_bits, packed, finish_from=None):
    """pushes ``meas[:, :finish_from]`` in pieces of ``sizes``, finishes with the rest; -> (list of push results, finish result)"""
    finish_from = synd_bits if finish_from is None else finish_from
    out, pos = [], 0
    for k in sizes:
        k = min(k, finish_from - pos)
        out.append(push(*as_chunk(meas[:, pos:pos + k], packed)))
        pos += k
    assert pos == finish_from
    return out, finish(*as_chunk(meas[:, pos:], packed))


@pytest.mark.parametrize("B", [1, 65, 96])
@pytest.mark.parametrize("tag", ["bb72", "shyps", "rep5"])
def test_front_end_equals_the_host_statement(tag, B):
    """every chunking, packed and unpacked, through ONE handle: each ``begin`` starts from a clean carry"""
    from slidingwindowdecoder_amd import MeasurementFrontEnd
    mm, h, mpr, meas, det, raw = record_case(tag)
    fe = MeasurementFrontEnd(mm, h, SHOTS)
    synd = fe.blocks.rounds * mpr
    nbytes = fe.device_bytes
    for name, sizes in bit_chunkings(synd, mpr).items():
        for packed in (False, True):
            fe.begin(B)
            rows, (last, got_raw) = feed(fe.push, fe.finish, meas[:B], sizes, synd, packed)
            done = 0
            for k, r in zip(np.cumsum(sizes), rows):  # each push returned exactly the rounds it completed
                assert r.shape == (B, k // mpr * h - done), (name, packed)
                done = k // mpr * h
            assert np.array_equal(np.concatenate(rows + [last], axis=1), det[:B]), (name, packed)
            assert np.array_equal(got_raw, raw[:B]), (name, packed)
            assert fe.bits_received == mm.num_meas and fe.rounds_done == fe.blocks.rounds
    # a finish that brings whole further rounds: after one round, and from inside the second, the rest of the record at once
    for first in (mpr, mpr + 5, 3):
        for packed in (False, True):
            fe.begin(B)
            rows, (last, got_raw) = feed(fe.push, fe.finish, meas[:B], [first], synd, packed, finish_from=first)
            assert rows[0].shape == (B, first // mpr * h) and last.shape == (B, det.shape[1] - first // mpr * h)
            assert np.array_equal(np.concatenate(rows + [last], axis=1), det[:B]), (first, packed)
            assert np.array_equal(got_raw, raw[:B]), (first, packed)
    # a byte chunk of another dtype: every non-zero value is a 1, as on the device (256 is not 0)
    fe.begin(B)
    wide = meas[:B].astype(np.int64) * np.array([1, 2, 256, 255, 65536], np.int64)[np.arange(mm.num_meas) % 5]
    rows = fe.push(wide[:, :synd])
    last, got_raw = fe.finish(wide[:, synd:])
    assert np.array_equal(np.concatenate([rows, last], axis=1), det[:B]) and np.array_equal(got_raw, raw[:B])
    assert fe.device_bytes == nbytes  # the state does not grow with what has been pushed
    fe.close()


@functools.lru_cache(maxsize=None)
def long_record(R, B):
    """(map of rep_code(5) at R rounds, a random record [B, 4 R + 5], its detectors, its raw observables); shared, read-only"""
    from slidingwindowdecoder_amd import measurements as ms
    from slidingwindowdecoder_amd.codes import rep_code
    mm = ms.phenomenological_measurement_map(rep_code(5), np.ones((1, 5), np.uint8), R)
    meas = np.random.default_rng(SEED).integers(0, 2, (B, mm.num_meas)).astype(np.uint8)
    det, obs = ms.detectors_from_measurements_host(mm, meas)
    for a in (meas, det, obs):
        a.setflags(write=False)
    return mm, meas, det, obs


@pytest.mark.parametrize("packed", [False, True])
def test_a_push_longer_than_one_launch_stages(packed):
    """rep_code(5) at 8300 rounds: one push of 33 200 bits is cut into two launches (a launch stages 32 768 bytes), the second
    starting at bit 32 762 of the buffer -- inside a byte of a packed chunk; then a finish that brings 99 whole rounds"""
    from slidingwindowdecoder_amd import MeasurementFrontEnd
    from slidingwindowdecoder_amd import measurements as ms
    R, B = 8400, 3
    mm, meas, det, obs = long_record(R, B)
    fe = MeasurementFrontEnd(mm, 4, B)
    fe.begin(B)
    long = 8300 * 4
    rows, (last, raw) = feed(fe.push, fe.finish, meas, [2, long], 4 * R, packed, finish_from=2 + long)
    assert rows[1].shape == (B, long) and last.shape == (B, det.shape[1] - long)
    assert np.array_equal(np.concatenate(rows + [last], axis=1), det)
    assert np.array_equal(raw, ms.observable_masks(obs)) and det.any()
    fe.close()


def test_front_end_device_form_aligned_and_unaligned_buffers():
    """``push_device`` / ``finish_device`` on column slices of one tensor (pointers off the 8-byte grid, byte loads) and on padded
    tensors of their own (8-byte loads), bytes and bits, on a side stream"""
    import torch
    from slidingwindowdecoder_amd import MeasurementFrontEnd
    mm, h, mpr, meas, det, raw = record_case("shyps")
    fe = MeasurementFrontEnd(mm, h, SHOTS)
    synd = fe.blocks.rounds * mpr
    side = torch.cuda.Stream()
    whole = torch.from_numpy(meas.copy()).cuda()
    torch.cuda.synchronize()
    cuts = [0, 5, 98, 199, 303, synd]
    for mode in ("slices", "padded", "packed", "packed-padded"):
        fe.begin(SHOTS)
        rows = []

        def dev(lo, hi):
            bits = meas[:, lo:hi]
            if mode == "slices":
                return whole[:, lo:hi], False
            a = np.packbits(bits, axis=1, bitorder="little") if mode.startswith("packed") else bits
            if mode.endswith("padded"):  # rows 8-byte aligned: every shot's buffer takes the vector path
                t = torch.zeros((SHOTS, (a.shape[1] + 7) // 8 * 8 + 8), dtype=torch.uint8, device="cuda")
                t[:, :a.shape[1]] = torch.from_numpy(np.array(a)).cuda()
                torch.cuda.synchronize()
                return t[:, :a.shape[1]], (hi - lo if mode.startswith("packed") else False)
            return torch.from_numpy(np.array(a)).cuda(), (hi - lo if mode.startswith("packed") else False)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            t, packed = dev(lo, hi)
            torch.cuda.synchronize()
            rows.append(fe.push_device(t, packed, stream=side))
        t, packed = dev(synd, mm.num_meas)
        torch.cuda.synchronize()
        last, got_raw = fe.finish_device(t, packed, stream=side)
        side.synchronize()
        got = np.concatenate([r.cpu().numpy() for r in rows + [last]], axis=1)
        assert np.array_equal(got, det), mode
        assert np.array_equal(got_raw.cpu().numpy().astype(np.uint32), raw), mode
    fe.close()


@functools.lru_cache(maxsize=None)
def experiment(rounds):
    """[[72,12,6]], p = 0.004, (3, 1, method 1), seed 13, 96 shots -- the experiment of tests/test_gpu_session.py (6 rounds) and of
    tests/test_gpu_rolling.py (its template at 6 rounds; 9 rounds): (plan, map of this length, det, true observable masks, a
    measurement record with these detectors and raw parities).  On the CPU: every one of the 96 shots has a true observable flip
    at both lengths."""
    from slidingwindowdecoder_amd import measurements as ms
    from slidingwindowdecoder_amd.circuit import bb_memory_ops
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import sample_dem
    from tests.test_rolling_host import plan_for
    plan = plan_for("w3f1m1", rounds)
    det, obs, _ = sample_dem(plan.chk, plan.obs, plan.priors, SHOTS, seed=SEED)
    code, A, B = bb_code(72)
    mm = ms.measurement_map(bb_memory_ops(code, A, B, 0.004, rounds), 36)
    meas = ms.synthesize_measurements_host(mm, det, obs, np.random.default_rng(SEED))
    d, o = ms.detectors_from_measurements_host(mm, meas)
    assert np.array_equal(d, det) and np.array_equal(o, obs)
    true_flips = ms.observable_masks(obs)
    for a in (det, true_flips, meas):
        a.setflags(write=False)
    return plan, mm, det, true_flips, meas


def same_events(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w) and g[0] == w[0]
        for x, y in zip(g[1:], w[1:]):
            assert np.array_equal(x, y), f"window {g[0]}"


@pytest.mark.parametrize("packed", [False, True])
def test_fixed_measurement_session(packed):
    """the plan, KW, seed and shots of tests/test_gpu_session.py: every push returns the events of ``session.push`` of the rows it
    completed, ``finish`` equals ``decode``, and the corrected readout is the true flips XOR the predicted ones.  All 96 shots of
    seed 13 have a true observable flip (checked with ``sample_dem`` on the CPU)."""
    from tests.test_gpu_session import assert_equals_decode, one_launch, problem
    plan, mm, det, true_flips, meas = experiment(6)
    _, det_s, _ = problem("w3f1m1")
    assert np.array_equal(det, det_s)
    dec, ref = one_launch("w3f1m1")
    assert true_flips.any() and (true_flips != 0).sum() == SHOTS
    ms_, ses = dec.measurement_session(SHOTS, mm), dec.session(SHOTS)
    h, mpr, synd = 36, 72, 6 * 72
    for name, sizes in bit_chunkings(synd, mpr).items():
        ms_.begin(SHOTS)
        ses.begin(SHOTS)
        events, fin = feed(ms_.push, ms_.finish, meas, sizes, synd, packed)
        done = 0
        for k, ev in zip(np.cumsum(sizes), events):
            same_events(ev, ses.push(det[:, done:k // mpr * h]))
            done = k // mpr * h
        same_events(ms_.last_events, ses.push(det[:, done:]))
        assert [e[0] for ev in events for e in ev] + [e[0] for e in ms_.last_events] == list(range(len(plan.windows))), name
        assert_equals_decode(fin[:5], ref)
        assert_equals_decode(ses.finish(), ref)
        raw, logical = fin[5], fin[6]
        assert np.array_equal(raw, true_flips), name
        assert np.array_equal(logical, true_flips ^ ref[3]), name
    assert ref[3].any() and not np.array_equal(ref[3], true_flips)  # some shots are corrected, some end in a logical error
    ms_.close()
    ses.close()


def test_fixed_measurement_session_device_form():
    import torch
    from tests.test_gpu_session import assert_equals_decode, one_launch, ready_windows
    plan, mm, det, true_flips, meas = experiment(6)
    dec, ref = one_launch("w3f1m1")
    ms_ = dec.measurement_session(SHOTS, mm)
    ms_.begin(SHOTS)
    dev = torch.from_numpy(meas.copy()).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    cuts, rows = [0, 50, 72, 250, 251, 432], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        first, count = ms_.push_device(dev[:, lo:hi], stream=side)
        assert list(range(first, first + count)) == ready_windows(plan, rows, hi // 72 * 36)
        rows = hi // 72 * 36
    side.synchronize()
    fin = ms_.finish(meas[:, 432:])
    assert_equals_decode(fin[:5], ref)
    assert np.array_equal(fin[6], true_flips ^ ref[3])
    ms_.close()


def test_pushes_on_alternating_streams_and_a_finish_with_whole_rounds():
    """``push_device`` takes its stream per call: consecutive pushes alternate between two streams with no host wait in between, so
    the front end's launch of one push is queued while the window decode of the push before still runs on the other stream -- the
    rows of a push must not be overwritten before the session's merge has read them.  Both sessions; then ``finish`` with the last
    two rounds and the final block at once.  Expected values: ``decode`` and the true flips."""
    import torch
    from tests.test_gpu_rolling import one_launch as rolling_ref, template_decoder
    from tests.test_gpu_session import assert_equals_decode, one_launch
    plan, mm, det, true_flips, meas = experiment(6)
    dec, ref = one_launch("w3f1m1")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = torch.from_numpy(meas.copy()).cuda()
    torch.cuda.synchronize()
    fixed = dec.measurement_session(SHOTS, mm)
    rolling = template_decoder("w3f1m1").rolling_measurement_session(SHOTS, mm)
    for rep in range(3):
        for ses in (fixed, rolling):
            ses.begin(SHOTS)
            for r in range(4):  # one round per push, the streams in turn, nothing waited for
                ses.push_device(dev[:, 72 * r:72 * (r + 1)], stream=streams[r & 1])
            fin = ses.finish(meas[:, 288:])  # rounds 4 and 5 and the final block
            if ses is fixed:
                assert_equals_decode(fin[:5], ref)
                assert np.array_equal(fin[6], true_flips ^ ref[3])
            else:
                rref = rolling_ref("w3f1m1", 6)
                assert np.array_equal(fin[4], rref[3]) and np.array_equal(fin[5], rref[4])
                assert np.array_equal(fin[6], true_flips) and np.array_equal(fin[7], true_flips ^ rref[3])
                assert len(ses.last_events) == 2  # the two windows that rounds 4 and 5 completed
    fixed.close()
    rolling.close()


@pytest.mark.parametrize("rounds", [6, 9])
def test_rolling_measurement_session(rounds):
    """the template of tests/test_gpu_rolling.py at R0 = 6 and R0 + 3 rounds: fed the record, the rolling measurement session returns
    what the rolling session returns for the host-derived rows; ``finish`` gets the second half of the last syndrome round together
    with the final block"""
    from tests.test_gpu_rolling import one_launch, template_decoder
    _, mm0, _, _, _ = experiment(6)  # the map of the template's own length
    plan, mm, det, true_flips, meas = experiment(rounds)
    ref = one_launch("w3f1m1", rounds)
    dec = template_decoder("w3f1m1")
    rm, rs = dec.rolling_measurement_session(SHOTS, mm0), dec.rolling_session(SHOTS)
    h, mpr, synd = 36, 72, rounds * 72
    stop = synd - 30  # inside the last syndrome round
    for name, sizes in bit_chunkings(stop, mpr).items():
        for packed in (False, True):
            rm.begin(SHOTS)
            rs.begin(SHOTS)
            events, fin = feed(rm.push, rm.finish, meas, sizes, synd, packed, finish_from=stop)
            done = 0
            for k, ev in zip(np.cumsum(sizes), events):
                same_events(ev, rs.push(det[:, done:k // mpr * h]))
                done = k // mpr * h
            assert done == (rounds - 1) * h
            same_events(rm.last_events, rs.push(det[:, done:-h]))  # the round that finish completed
            want = rs.finish(det[:, -h:])
            assert fin[0] == want[0] == len(plan.windows) - 1
            for x, y in zip(fin[1:6], want[1:]):
                assert np.array_equal(x, y), name
            assert np.array_equal(fin[4], ref[3]) and np.array_equal(fin[5], ref[4])
            assert np.array_equal(fin[6], true_flips) and np.array_equal(fin[7], true_flips ^ ref[3])
    rm.close()
    rs.close()


def test_refusals_leave_the_session_usable():
    from slidingwindowdecoder_amd import measurements as ms
    from tests.test_gpu_rolling import template_decoder
    from tests.test_gpu_session import assert_equals_decode, one_launch
    plan, mm, det, true_flips, meas = experiment(6)
    dec, ref = one_launch("w3f1m1", 4)
    B = 4
    # a map that does not fit the plan: another number of rows per round, another number of rounds
    from slidingwindowdecoder_amd.shyps import shyps_memory_ops
    other = ms.measurement_map(shyps_memory_ops(3, 0.002, 11), 21)
    assert other.det.shape[0] == 252  # (the row count alone fits)
    with pytest.raises(ValueError, match="the map has 21 detector rows per round, the plan 36"):
        dec.measurement_session(B, other)
    with pytest.raises(ValueError, match="the map has 360 detectors, the plan 252"):
        dec.measurement_session(B, experiment(9)[1])
    with pytest.raises(ValueError, match="the map has 21 detector rows per round, the plan 36"):
        template_decoder("w3f1m1").rolling_measurement_session(B, other)
    # a map that does not carry its rows per round is cut by the plan's: one more detector row leaves no whole blocks
    import scipy.sparse as sp
    ragged = ms.MeasurementMap(sp.vstack([mm.det, mm.det[:1]], format="csr"), mm.obs, mm.num_meas)
    with pytest.raises(ValueError, match="the map has 253 detectors, the plan 252"):
        dec.measurement_session(B, ragged)
    with pytest.raises(ValueError, match="253 detector rows are not"):
        template_decoder("w3f1m1").rolling_measurement_session(B, ragged)
    ses = dec.measurement_session(B, mm)
    ses.begin(B)
    assert ses.push(meas[:B, :100]) == []
    with pytest.raises(ValueError, match=r"333 bits after 100 received: the syndrome rounds of this experiment have 432"):
        ses.push(meas[:B, 100:433])
    with pytest.raises(ValueError, match=r"finish: 72 bits after 100 received"):
        ses.finish(meas[:B, 432:])  # the last syndrome round is not complete
    with pytest.raises(ValueError, match="a packed chunk of 9 bits is 2 bytes wide"):
        ses.push(np.zeros((B, 1), np.uint8), packed=9)
    assert ses.bits_received == 100
    events = ses.push(meas[:B, 100:400])
    fin = ses.finish(meas[:B, 400:])
    assert [e[0] for e in events] + [e[0] for e in ses.last_events] == list(range(len(plan.windows)))
    assert_equals_decode(fin[:5], ref)
    assert np.array_equal(fin[6], true_flips[:B] ^ ref[3])
    ses.close()
    # rolling: a finish that does not end the round under way, and a length the template does not serve (4 rounds: 6 = 4 (mod 1)
    # would fit (3, 1); two rounds are fewer than head and tail need)
    rm = template_decoder("w3f1m1").rolling_measurement_session(B, mm)
    rm.begin(B)
    rm.push(meas[:B, :100])
    with pytest.raises(ValueError, match="do not complete the last syndrome round"):
        rm.finish(meas[:B, 432:])
    with pytest.raises(ValueError, match="this template serves"):
        rm.finish(meas[:B, 388:])  # 44 + 72 bits: ends round 1 and brings a final block -- two syndrome rounds
    assert rm.bits_received == 100
    rm.push(meas[:B, 100:420])
    fin = rm.finish(meas[:B, 420:])
    assert np.array_equal(fin[4], ref[3]) and np.array_equal(fin[7], true_flips[:B] ^ ref[3])
    rm.close()
