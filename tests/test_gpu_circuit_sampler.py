"""The device circuit sampler (``CircuitSampler``, C ABI swd_circuit_sampler_*) against the host statement of the Pauli-frame rule
(``frames.simulate_frames_host`` fed with the streams as tests/frame_ref.py restates them): every bit of the record, the detectors
and observable masks as parities of it, the marginals of the detector error model, the record through the measurement session,
and ``MemoryExperiment`` drawing its shots from the circuit.  Expected values never come from the device.  All comparisons are
exact but the marginals, which are held to a binomial bound."""
import functools

import numpy as np
import pytest

from tests import frame_ref
from tests.test_frames_host import circuit_ops, dem_marginals
from tests.test_session_host import KW

pytestmark = pytest.mark.gpu

SEED = 20240318
WRAP = (1 << 32) - 3  # the high word of the shot number changes inside a batch that starts here
CASES = ["bb72z", "bb72x", "shyps3", "hand"]


def ops_of(tag):
    return frame_ref.hand_written_ops() if tag == "hand" else circuit_ops(tag)


@functools.lru_cache(maxsize=None)
def host_case(tag, randomize, first_shot, shots):
    """(map, record [shots, num_meas], det, observable masks) of the host statement; shared, read-only"""
    from slidingwindowdecoder_amd import measurements as ms
    ops = ops_of(tag)
    mm = ms.measurement_map(ops)
    rec = frame_ref.records(ops, shots, SEED, first_shot, randomize)
    det, obs = ms.detectors_from_measurements_host(mm, rec)
    masks = ms.observable_masks(obs)
    for a in (rec, det, masks):
        a.setflags(write=False)
    return mm, rec, det, masks


@functools.lru_cache(maxsize=None)
def sampler_of(tag, randomize=True):
    from slidingwindowdecoder_amd import CircuitSampler
    return CircuitSampler(ops_of(tag), randomize=randomize)


def test_hand_written_list_uses_every_op_kind_and_every_pauli():
    from slidingwindowdecoder_amd.circuit import DEP1, DEP2, DETECTOR, OBSERVABLE
    from slidingwindowdecoder_amd.frames import OP_NAMES, compile_ops
    prog = compile_ops(frame_ref.hand_written_ops())
    assert set(prog.kind.tolist()) == set(OP_NAMES) - {DETECTOR, OBSERVABLE} and prog.num_qubits == 5
    codes = frame_ref.pauli_codes(prog, 200, SEED, WRAP)
    slots = {k: prog.noise_slot[prog.kind == k] for k in (DEP1, DEP2)}
    assert set(codes[:, slots[DEP2]].ravel().tolist()) == set(range(16))  # all 15 two-qubit Paulis, and none
    assert set(codes[:, slots[DEP1]].ravel().tolist()) == set(range(4))


@pytest.mark.parametrize("randomize", [True, False])
@pytest.mark.parametrize("tag", CASES)
def test_record_equals_the_host_statement(tag, randomize):
    import torch
    s = sampler_of(tag, randomize)
    mm, rec, det, masks = host_case(tag, randomize, WRAP, 200)
    assert s.num_meas == mm.num_meas == rec.shape[1] and rec.any()
    if tag == "shyps3":
        assert s.num_meas == 245  # no whole number of bytes
    got = s.measure(200, SEED, WRAP)
    assert got.dtype == np.uint8 and np.array_equal(got, rec)
    assert ((WRAP + 199) >> 32) == 1
    # packed equals unpacked
    assert np.array_equal(s.measure(200, SEED, WRAP, packed=True), np.packbits(rec, axis=1, bitorder="little"))
    # batches of 1, 63, 65: the last wave is partly empty, a second wave holds one shot
    _, rec7, _, _ = host_case(tag, randomize, 7, 65)
    for shots in (1, 63, 65):
        assert np.array_equal(s.measure(shots, SEED, 7), rec7[:shots]), shots
    # independence of batching: 77 + 123 shots in two calls
    a, b = s.measure(77, SEED, WRAP), s.measure(123, SEED, WRAP + 77)
    assert np.array_equal(np.concatenate([a, b]), rec)
    # the device form: a padded caller buffer keeps its padding, bytes and bits
    for packed in (False, True):
        row = s.record_bytes(packed)
        buf = torch.full((202, row + 11), 0xA5, dtype=torch.uint8, device="cuda")
        out = s.measure_device(200, SEED, WRAP, packed=packed, out=buf[1:, 3:])
        assert out.shape == (200, row) and out.data_ptr() == buf[1:, 3:].data_ptr()
        h = buf.cpu().numpy()
        want = np.packbits(rec, axis=1, bitorder="little") if packed else rec
        assert np.array_equal(h[1:201, 3:3 + row], want), packed
        h[1:201, 3:3 + row] = 0xA5
        assert (h == 0xA5).all(), packed
    assert np.array_equal(s.measure_device(65, SEED, 7).cpu().numpy(), rec7)
    # another seed is another record
    assert not np.array_equal(s.measure(65, SEED + 1, 7), rec7)


@pytest.mark.parametrize("randomize", [True, False])
@pytest.mark.parametrize("tag", CASES)
def test_sample_equals_the_host_map_of_the_record(tag, randomize):
    import torch
    s = sampler_of(tag, randomize)
    mm, rec, det, masks = host_case(tag, randomize, WRAP, 200)
    assert s.num_det == det.shape[1] and det.any() and masks.any()
    d, f = s.sample_device(200, SEED, WRAP)
    assert d.dtype == torch.uint8 and f.dtype == torch.int32
    assert np.array_equal(d.cpu().numpy(), det) and np.array_equal(f.cpu().numpy().view(np.uint32), masks)
    # caller's tensors with room to spare, the record along with it, on a side stream; without masks
    side = torch.cuda.Stream()
    dd = torch.full((210, s.num_det), 7, dtype=torch.uint8, device="cuda")
    ff = torch.full((210,), -1, dtype=torch.int32, device="cuda")
    mmeas = torch.full((200, s.num_meas + 5), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d2, f2 = s.sample_device(200, SEED, WRAP, out=(dd, ff), stream=side, meas=mmeas)
    side.synchronize()
    assert np.array_equal(d2.cpu().numpy(), det) and np.array_equal(f2.cpu().numpy().view(np.uint32), masks)
    assert (dd[200:] == 7).all() and (ff[200:] == -1).all() and (mmeas[:, s.num_meas:] == 7).all()
    assert np.array_equal(mmeas[:, :s.num_meas].cpu().numpy(), rec)
    d3, f3 = s.sample_device(63, SEED, WRAP, out=(dd, None))
    assert f3 is None and np.array_equal(d3.cpu().numpy(), det[:63])
    # the host-pointer form
    hd, ho, hm = s.sample(200, SEED, WRAP, return_measurements=True)
    assert np.array_equal(hd, det) and np.array_equal(hm, rec)
    assert np.array_equal((ho.astype(np.uint32) << np.arange(ho.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32), masks)
    if not randomize:  # detectors and observables of a memory circuit do not depend on the mode (the hand-written list declares arbitrary parities)
        other = host_case(tag, True, WRAP, 200)
        assert not np.array_equal(other[1], rec)
        if tag != "hand":
            assert np.array_equal(other[2], det) and np.array_equal(other[3], masks)
    info = s.info()
    assert (info["qubits"], info["measurements"], info["detectors"], info["observables"]) == (s.num_qubits, s.num_meas, s.num_det, s.num_obs)
    assert info["noise_slots"] == s.program.num_noise and info["random_slots"] == s.program.num_rand and info["max_qubits"] == 4096
    assert info["device_bytes"] >= 16 * len(s.program) + 8 * 4 * s.num_meas


def test_marginals_equal_the_dem():
    """32 768 shots of [[72,12,6]] z, 3 rounds, p = 0.01: every detector's and observable's frequency within 5 sigma of
    P = (1 - prod(1 - 2 p_j)) / 2 over the DEM columns touching it, sigma = sqrt(P (1 - P) / N): a binomial bound.  The host
    statement at this seed lies within 2.78 sigma (tests/test_frames_host.py::test_host_marginals_equal_the_dem)."""
    N = 32768
    P = dem_marginals(circuit_ops("bb72z"))
    det, obs = sampler_of("bb72z").sample(N, SEED, 0)
    freq = np.concatenate([det, obs], axis=1).mean(axis=0)
    dev = np.abs(freq - P) / np.sqrt(P * (1.0 - P) / N)
    print(f"largest deviation {dev.max():.2f} sigma over {len(P)} rows")
    assert len(P) == 156 and dev.max() <= 5.0


@functools.lru_cache(maxsize=None)
def bb72_rounds4():
    """(ops, plan) of bb(72, 0.004, 4, 3, 1)"""
    from slidingwindowdecoder_amd.circuit import bb_dem, bb_memory_ops
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, 4)
    return bb_memory_ops(code, A, B, 0.004, 4), plan_windows(dem.chk, dem.obs, dem.priors, 36, 3, 1, 1, True)


def test_record_through_the_measurement_session():
    """64 shots' packed records from ``measure_device`` into ``measurement_session``: the first piece straight from the sampler's
    tensor (100 bits: it ends inside round 1 and inside byte 12), the rest cut at bits 171 and 288 and repacked -- a packed chunk
    starts at bit 0 of its buffer -- then ``finish``.  Expected: ``decode`` of the detectors the host map gives"""
    import torch
    from slidingwindowdecoder_amd import CircuitSampler, SlidingWindowDecoder
    from slidingwindowdecoder_amd import measurements as ms
    from tests.test_gpu_session import assert_equals_decode
    ops, plan = bb72_rounds4()
    B = 64
    s = CircuitSampler(ops, n_half=36)
    assert s.num_meas == 360 and s.mmap.n_half == 36
    rec = frame_ref.records(ops, B, SEED, 0, True)
    det, obs = ms.detectors_from_measurements_host(s.mmap, rec)
    raw = ms.observable_masks(obs)
    dec = SlidingWindowDecoder(plan, **KW)
    total = dec.decode(det).copy()
    ref = (total, dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())
    side = torch.cuda.Stream()
    packed = s.measure_device(B, SEED, 0, packed=True, stream=side)
    side.synchronize()
    assert packed.shape == (B, 45) and np.array_equal(packed.cpu().numpy(), np.packbits(rec, axis=1, bitorder="little"))
    ses = dec.measurement_session(B, s.mmap)
    ses.begin(B)
    ses.push_device(packed[:, :13], packed=100, stream=side)
    side.synchronize()
    bits = np.unpackbits(packed.cpu().numpy(), axis=1, bitorder="little")[:, :360]
    for lo, hi in ((100, 171), (171, 288)):
        ses.push(np.packbits(bits[:, lo:hi], axis=1, bitorder="little"), packed=hi - lo)
    fin = ses.finish(np.packbits(bits[:, 288:], axis=1, bitorder="little"), packed=72)
    assert_equals_decode(fin[:5], ref)
    assert np.array_equal(fin[5], raw) and raw.any()
    assert np.array_equal(fin[6], raw ^ fin[3]) and np.array_equal(fin[6], raw ^ ref[3])
    ses.close()
    s.close()


@functools.lru_cache(maxsize=None)
def circuit_specification(shots=256):
    """what ``memory_experiment_host`` makes of the host statement's shots, the oracle in the windows"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import measurements as ms
    from slidingwindowdecoder_amd.windows import memory_experiment_host
    ops, plan = bb72_rounds4()
    det, obs = ms.detectors_from_measurements_host(ms.measurement_map(ops), frame_ref.records(ops, shots, SEED, 0, True))
    return memory_experiment_host(plan, det, obs, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))


def test_memory_experiment_samples_the_circuit():
    from slidingwindowdecoder_amd import CircuitSampler, MemoryExperiment
    from tests.test_memory_experiment_host import as_result
    want = as_result(circuit_specification())
    assert want.shots == 256 and want.logical_errors > 0
    exp = MemoryExperiment.bb(72, 0.004, 4, 3, 1, sampler="circuit", **KW)
    assert isinstance(exp.sampler, CircuitSampler) and exp.sampler.num_det == exp.plan.chk.shape[0] == 180
    for batch, lanes in ((100, 1), (100, 2), (256, 2)):
        got = exp.run(256, batch=batch, lanes=lanes, keep_failures=256)
        print(batch, lanes, got)
        assert got == want, (batch, lanes)
    exp.close()


def test_default_memory_experiment_is_unchanged():
    """``sampler=None``: the DEM sampler's shots, as ``memory_experiment_host`` decodes them with the oracle in the windows"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import DemSampler, MemoryExperiment
    from slidingwindowdecoder_amd.windows import memory_experiment_host
    from tests.test_memory_experiment_host import as_result, sample
    _, plan = bb72_rounds4()
    det, obs, _ = sample(plan, 256, SEED)
    want = as_result(memory_experiment_host(plan, det, obs, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW)))
    exp = MemoryExperiment.bb(72, 0.004, 4, 3, 1, **KW)
    assert isinstance(exp.sampler, DemSampler)
    assert exp.run(256, batch=100, keep_failures=256) == want
    assert want != as_result(circuit_specification())  # (the two samplers draw different shots)
    exp.close()


def test_refusals():
    import torch
    from slidingwindowdecoder_amd import CapacityError, CircuitSampler, MemoryExperiment
    from slidingwindowdecoder_amd.circuit import DETECTOR, M, OBSERVABLE, R
    # the qubit bound: 4096 qubits fit a wave's 64 KB of LDS, 4097 do not
    ok = CircuitSampler([(R, 4095), (M, 4095, 0), (DETECTOR, (0,))], randomize=False)
    assert ok.info()["qubits"] == 4096 and not ok.measure(3, SEED).any()
    with pytest.raises(CapacityError, match="4097 qubits"):
        CircuitSampler([(R, 4096), (M, 4096, 0)])
    # more than 32 observables: records and detectors are served, observable masks are not
    many = CircuitSampler([(R, 0), (M, 0, 0), (DETECTOR, (0,))] + [(OBSERVABLE, (0,))] * 33)
    assert many.measure(2, SEED).shape == (2, 1)
    assert many.sample_device(2, SEED, out=(torch.empty((2, 1), dtype=torch.uint8, device="cuda"), None))[1] is None
    with pytest.raises(CapacityError, match="32 observables"):
        many.sample_device(2, SEED)
    with pytest.raises(CapacityError, match="32 observables"):
        many.sample(2, SEED)
    # a sampler whose detector count does not fit the plan
    _, plan = bb72_rounds4()
    with pytest.raises(ValueError, match="the sampler draws 144 detectors, the plan has 180"):
        MemoryExperiment(plan, sampler=sampler_of("bb72z"), **KW)
    with pytest.raises(ValueError, match="sampler"):
        MemoryExperiment.bb(72, 0.004, 4, 3, 1, sampler="stim", **KW)
    with pytest.raises(ValueError, match="sample_device"):
        MemoryExperiment(plan, sampler=object(), **KW)
    # tensors on the wrong device, of the wrong type, too small
    s = sampler_of("hand")
    good = lambda: (torch.empty((4, s.num_det), dtype=torch.uint8, device="cuda"), torch.empty((4,), dtype=torch.int32, device="cuda"))  # noqa: E731
    with pytest.raises(ValueError, match="det lives on cpu"):
        s.sample_device(4, SEED, out=(torch.empty((4, s.num_det), dtype=torch.uint8), good()[1]))
    with pytest.raises(ValueError, match="flips lives on cpu"):
        s.sample_device(4, SEED, out=(good()[0], torch.empty((4,), dtype=torch.int32)))
    with pytest.raises(ValueError, match="out lives on cpu"):
        s.measure_device(4, SEED, out=torch.empty((4, s.num_meas), dtype=torch.uint8))
    with pytest.raises(ValueError, match="meas lives on cpu"):
        s.sample_device(4, SEED, out=good(), meas=torch.empty((4, s.num_meas), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        s.measure_device(4, SEED, out=torch.empty((4, s.num_meas - 1), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        s.measure_device(5, SEED, out=torch.empty((4, s.num_meas), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="det must be"):
        s.sample_device(4, SEED, out=(torch.empty((4, s.num_det), dtype=torch.int32, device="cuda"), good()[1]))
    with pytest.raises(ValueError, match="out must be"):
        s.measure_device(4, SEED, out=torch.empty((s.num_meas, 4), dtype=torch.uint8, device="cuda").t())
