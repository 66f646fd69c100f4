"""Python class surface of the reference, backed by the HIP library.

``osd_window`` keeps the constructor kwargs, ``decode`` and the properties of the reference's
Cython class (/root/reference/src/osd_window.pyx:8-126, 158-199, 487-517) so that the
notebook / script loops (/root/reference/osd.py:152-167) run unchanged, and adds
``decode_batch`` (shape modelled on the batched decoders the reference's notebooks compare
against) which is the path that actually uses the GPU well: one launch, one workgroup per
syndrome.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib

EXIT_PRE, EXIT_POST, EXIT_OSD, EXIT_FAIL_SET, EXIT_FAIL_PEEL, EXIT_NO_OSD, EXIT_SCHED_FAULT = range(7)
STATUS_CONVERGE = 0x100

_OSD_METHODS = {  # aliases of osd_window.pyx:69-79
    0: ["osd_0", "0", "osd0"],
    1: ["osd_e", "1", "osde", "exhaustive", "e"],
    2: ["osd_cs", "2", "osdcs", "combination_sweep", "cs"],
}


def _parse_osd_method(osd_method, osd_order):
    s = str(osd_method).lower()
    for k, names in _OSD_METHODS.items():
        if s in names:
            return k, (0 if k == 0 else int(osd_order))
    raise ValueError(f"ERROR: OSD method '{osd_method}' invalid. Please choose from the following "
                     "methods: 'OSD_0', 'OSD_E' or 'OSD_CS'.")


class _Csr:
    """Validated CSR + priors kept alive for the C call."""

    def __init__(self, pcm, channel_probs):
        if not (isinstance(pcm, np.ndarray) or sp.issparse(pcm)):
            raise TypeError("The input matrix is of an invalid type. Please input a np.ndarray or "
                            f"scipy.sparse.spmatrix object, not {type(pcm)}")
        a = sp.csr_matrix(pcm)
        a.data = (np.asarray(a.data) != 0).astype(np.uint8)
        a.eliminate_zeros()
        a.sort_indices()
        self.m, self.n = a.shape
        if channel_probs is None:
            raise ValueError("channel_probs is required")
        probs = np.ascontiguousarray(channel_probs, dtype=np.float64)
        if len(probs) != self.n:
            raise ValueError("The length of the channel probability vector must be eqaul to the "
                             f"block length n={self.n}.")
        self.row_ptr = np.ascontiguousarray(a.indptr, dtype=np.int32)
        self.col_idx = np.ascontiguousarray(a.indices, dtype=np.int32)
        self.probs = probs
        self.desc = _lib.GraphDesc(self.m, self.n, int(self.row_ptr[-1]), self.row_ptr.ctypes.data,
                                   self.col_idx.ctypes.data, probs.ctypes.data)


def _as_synd(x, m):
    x = np.asarray(x)
    if x.ndim != 1 or x.shape[0] != m:
        n_in = x.shape[0] if x.ndim >= 1 else 0
        raise ValueError(f"The input to the ldpc.bp_decoder.decode must be a syndrome (of length={m}). "
                         f"The inputted vector has length={n_in}. Valid formats are `np.ndarray` or "
                         "`scipy.sparse.spmatrix`.")
    return np.ascontiguousarray((x.astype(np.int64) & 0xFF).astype(np.uint8))  # C (char) cast, c_util.pyx:6-9


def _node_depth(L, name, handle):
    """1 if the handle's full-graph node pass took the depth-profiled form (a development build may predate the query: uniform)"""
    f = getattr(L, name, None)
    return bool(f(handle)) if f is not None and getattr(f, "argtypes", None) else False


class _Handle:
    """Owner of one library handle ``_h`` that the C function named ``_destroy`` releases."""
    _h = _destroy = None

    def _release(self):
        h = getattr(self, "_h", None)  # (a constructor that raised early has not set it)
        if h:
            try:
                getattr(_lib.lib(), self._destroy)(h)
            except Exception:  # interpreter shutdown: the module globals may be gone already
                pass
            self._h = None

    __del__ = _release


class osd_window(_Handle):
    """BP + OSD on a shortened window matrix (reference: src/osd_window.pyx)."""
    _destroy = "swd_osdw_destroy"

    def __init__(self, parity_check_matrix, **kwargs):
        L = _lib.lib()
        self._csr = _Csr(parity_check_matrix, kwargs.get("channel_probs"))
        self.m, self.n = self._csr.m, self._csr.n
        method, order = _parse_osd_method(kwargs.get("osd_method", "osd_0"), kwargs.get("osd_order", 0))
        new_n = kwargs.get("new_n", None)
        self.pre_max_iter = int(kwargs.get("pre_max_iter", 8))
        self.post_max_iter = int(kwargs.get("post_max_iter", 100))
        self.ms_scaling_factor = float(kwargs.get("ms_scaling_factor", 1.0))
        self.osd_method, self.osd_order = method, order
        self.device = int(kwargs.get("device", 0))
        p = _lib.OsdwParams(self.pre_max_iter, self.post_max_iter, self.ms_scaling_factor,
                            int(new_n) if new_n else 0, method, order)
        self._h = L.swd_osdw_create(C.byref(self._csr.desc), C.byref(p), self.device)
        if not self._h:
            raise _lib.error("swd_osdw_create")
        i = [C.c_int32() for _ in range(4)]
        L.swd_osdw_info(self._h, *[C.byref(x) for x in i])
        self.new_n, self.rank = i[2].value, i[3].value
        # "depth": the full-graph node pass serves the nodes by degree, a fixed depth per cache row (csrc/swd_variants.h); "uniform" otherwise
        self.node_pass = "depth" if _node_depth(L, "swd_osdw_node_depth", self._h) else "uniform"
        # per-object state the reference keeps between decodes
        self._hist = np.zeros((4, self.n), dtype=np.float64)
        self._last = dict(status=EXIT_PRE, iters=0, min_pm=0.0)
        self._bp_decoding = np.zeros(self.n, dtype=np.int64)
        self._osdw_decoding = np.zeros(self.n, dtype=np.int64)
        self._osd0_decoding = np.zeros(self.n, dtype=np.int64)

    @property
    def last_form(self):
        """The forms of the window kernels this decoder takes and the kernel kind of its most recent launch (include/swd.h,
        swd_osdw_last_form): the dict of ``window_forms`` with ``kind`` (-1 before the first launch), ``stream_serial`` and
        ``depth_launch`` filled in."""
        return _last_form("swd_osdw_last_form", self._h, 1)

    # ---- reference surface -------------------------------------------------------------
    def decode(self, input_vector):
        """One syndrome -> int64[n] (osd_window.pyx:158-199).  The LLR history persists between
        calls exactly like the reference object's."""
        s = _as_synd(input_vector, self.m)
        out = np.zeros(self.n, dtype=np.uint8)
        st = np.zeros(_lib.STAT_WORDS, np.int32)
        pm = np.zeros(1, np.float64)
        osd0 = np.zeros(self.n, dtype=np.uint8)
        bpd = np.zeros(self.n, dtype=np.uint8)
        rc = _lib.lib().swd_osdw_decode_batch(self._h, 1, s.ctypes.data, out.ctypes.data, st.ctypes.data,
                                              pm.ctypes.data, self._hist.ctypes.data, 1, osd0.ctypes.data, bpd.ctypes.data)
        if rc:
            raise _lib.error("swd_osdw_decode_batch")
        self._last = dict(status=int(st[0]), iters=int(st[1]), min_pm=float(pm[0]))
        res = out.astype(np.int64)
        if (int(st[0]) & 0xFF) == EXIT_OSD:
            self._osdw_decoding = res
            self._osd0_decoding = osd0.astype(np.int64)
            self._bp_decoding = bpd.astype(np.int64)  # the BP decisions the OSD started from (osd_window.pyx:499-501)
        else:
            self._bp_decoding = res
        return res

    def decode_batch(self, syndromes, return_history=False, return_osd0=False):
        """B syndromes [B, m] -> uint8 [B, n]; every shot starts from a zero LLR history (the state
        of a freshly constructed reference object).  Per-shot results are kept in
        ``last_status`` / ``last_iterations`` / ``last_min_pm`` (and ``last_history`` [B,4,n])."""
        s = np.asarray(syndromes)
        if s.ndim != 2 or s.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape [B, {self.m}]")
        s = np.ascontiguousarray((s.astype(np.int64) & 0xFF).astype(np.uint8))
        B = s.shape[0]
        out = np.zeros((B, self.n), dtype=np.uint8)
        st = np.zeros((B, _lib.STAT_WORDS), np.int32)
        pm = np.zeros(B, np.float64)
        hist = np.zeros((B, 4, self.n), np.float64) if return_history else None
        osd0 = np.zeros((B, self.n), np.uint8) if return_osd0 else None
        rc = _lib.lib().swd_osdw_decode_batch(self._h, B, s.ctypes.data, out.ctypes.data, st.ctypes.data,
                                              pm.ctypes.data, hist.ctypes.data if hist is not None else None, 0,
                                              osd0.ctypes.data if osd0 is not None else None, None)
        if rc:
            raise _lib.error("swd_osdw_decode_batch")
        self.last_stats = st
        self.last_status, self.last_iterations, self.last_min_pm = st[:, 0].copy(), st[:, 1].copy(), pm
        self.last_history, self.last_osd0 = hist, osd0
        return out

    def decode_batch_device(self, synd, out=None, stats=None, min_pm=None, stream=None):
        """Device-resident batch: ``synd`` is a torch uint8 CUDA tensor [B, m] (row stride free).
        Asynchronous on the current (or given) torch stream.  Returns (out, stats[B, 8], min_pm)
        tensors; stats[:, 0] = exit class | 0x100 * converge, stats[:, 1] = bp_iteration."""
        import torch
        B = synd.shape[0]
        dev = synd.device
        out = torch.empty((B, self.n), dtype=torch.uint8, device=dev) if out is None else out
        stats = torch.empty((B, _lib.STAT_WORDS), dtype=torch.int32, device=dev) if stats is None else stats
        min_pm = torch.empty(B, dtype=torch.float64, device=dev) if min_pm is None else min_pm
        st = torch.cuda.current_stream(dev) if stream is None else stream
        rc = _lib.lib().swd_osdw_decode_batch_dev(self._h, B, synd.data_ptr(), synd.stride(0), out.data_ptr(),
                                                  out.stride(0), stats.data_ptr(), min_pm.data_ptr(), None, 0, None, None,
                                                  st.cuda_stream)
        if rc:
            raise _lib.error("swd_osdw_decode_batch_dev")
        return out, stats, min_pm

    def set_timing(self, on=True):
        _lib.lib().swd_osdw_set_timing(self._h, 1 if on else 0)

    def get_timing(self):
        ms, k = C.c_double(), C.c_int64()
        _lib.lib().swd_osdw_get_timing(self._h, C.byref(ms), C.byref(k))
        return ms.value, k.value

    @property
    def bp_iteration(self):
        return self._last["iters"]

    @property
    def converge(self):
        return 1 if (self._last["status"] & STATUS_CONVERGE) else 0

    @property
    def min_pm(self):
        return self._last["min_pm"]

    @property
    def exit_class(self):
        return self._last["status"] & 0xFF

    @property
    def bp_decoding(self):
        return self._bp_decoding.copy()

    @property
    def osdw_decoding(self):
        return self._osdw_decoding.copy()

    @property
    def osd0_decoding(self):
        return self._osd0_decoding.copy()

    @property
    def log_prob_ratios(self):
        return np.ascontiguousarray(self._hist.T)


def hypotheses_shape(hyp):
    """(max_tree_depth D, max_side_depth S) of the decimation tree with exactly ``hyp`` root-to-leaf hypotheses per shot:
    leaves = 1 (main) + (S - D) (side branches below the tree) + 2 (2^D - 1) (two per tree node; bpgd.cpp:576-577,
    bp_guessing_decoder.pyx:181) with the deepest full tree that fits -- 64 -> D = 5, S = 6; 32 -> (4, 5); 16 -> (3, 4); 100 -> (5, 42).
    The device holds trees of depth <= 6 and at most 160 snapshots (2 (2^D - 1) + S - D)."""
    hyp = int(hyp)
    if hyp < 1:
        raise ValueError("hypotheses must be a positive integer")
    D = 0
    while D < 6 and 2 * (2 ** (D + 1) - 1) + 1 <= hyp:
        D += 1
    side = hyp - (2 * (2 ** D - 1) + 1)
    if 2 * (2 ** D - 1) + side > 160:
        raise ValueError(f"hypotheses={hyp}: the device holds at most 161 hypotheses per shot (tree depth 6 would need "
                         f"{2 * (2 ** D - 1) + side} snapshots, limit 160)")
    return D, D + side


def _gdg_params(kwargs, mode):
    """kwargs of bp_guessing_decoder.pyx:7-9, 162-171, 475-478.  ``hypotheses=H`` (not a reference kwarg) picks the tree
    shape with H hypotheses per shot (``hypotheses_shape``: 64 -> max_tree_depth 5, max_side_depth 6) and scores every leaf
    of gdg()'s tree (``multi_thread=2``, this package's own ensemble)."""
    kwargs = dict(kwargs)
    hyp = kwargs.pop("hypotheses", None)
    if hyp is not None:
        D, S_ = hypotheses_shape(hyp)
        kwargs.update(max_tree_depth=D, max_side_depth=S_, multi_thread=2)  # 2: every leaf of gdg()'s tree (not a reference mode)
    new_n = kwargs.get("new_n", None)
    return _lib.GdgParams(int(kwargs.get("max_iter", 50)), float(kwargs.get("ms_scaling_factor", 1.0)),
                          int(kwargs.get("max_iter_per_step", 6)), int(kwargs.get("max_step", 25)),
                          int(kwargs.get("max_tree_depth", 3)), int(kwargs.get("max_side_depth", 10)),
                          int(kwargs.get("max_tree_branch_step", 10)), int(kwargs.get("max_side_branch_step", 10)),
                          float(kwargs.get("gdg_factor", kwargs.get("gd_factor", 1.0))),
                          int(new_n) if new_n else 0, int(bool(kwargs.get("low_error_mode", False))), mode,
                          (2 if kwargs.get("multi_thread", False) == 2 else int(bool(kwargs.get("multi_thread", False)))) if mode == 0 else 0)


# ---- which forms of the window kernels a plan takes (include/swd.h, swd_window_forms / swd_*_last_form) ----
FORM_PLAN_FIELDS = ("nt", "vf", "dm", "kg", "sf", "big", "depth_fit", "lds_total", "gdg_parallel", "post_depth2", "general",
                    "kind", "stream_serial", "depth_launch")
FORM_WINDOW_FIELDS = ("lslot", "post_lds", "osd_lds", "owide_ring", "cs_own", "cs_par", "mask_bytes", "osd0", "post",
                      "split_t", "split_1", "split_2", "split_4", "split_need", "wm", "pads")
_FORM_NAMES = {"lslot": ("staged", "own", "none"),
               "osd0": ("osd0_quad", "osd0_wave_reg", "osd0_cols", "osd0_colsw", "osd0_block"),
               "post": ("sorted", "lists", "no_lists", "renumbered")}


def _form_dict(plan, wins):
    """The int32 records of include/swd.h as a dict with named fields; ``windows`` holds one dict per window (none in the general
    form).  ``lslot``, ``osd0`` and ``post`` are given by name (None where the record holds -1)."""
    out = {k: int(v) for k, v in zip(FORM_PLAN_FIELDS, plan)}
    out["windows"] = []
    for rec in (wins if not out["general"] else ()):
        w = {k: int(v) for k, v in zip(FORM_WINDOW_FIELDS, rec)}
        for k, names in _FORM_NAMES.items():
            w[k] = names[w[k]] if w[k] >= 0 else None
        out["windows"].append(w)
    return out


def _last_form(name, handle, nwin):
    plan = np.zeros(_lib.FORM_PLAN_WORDS, np.int32)
    wins = np.full((max(nwin, 1), _lib.FORM_WINDOW_WORDS), -1, np.int32)
    if getattr(_lib.lib(), name)(handle, plan.ctypes.data, wins.ctypes.data):
        raise _lib.error(name)
    return _form_dict(plan, wins[:nwin])


def window_forms(windows, decoder="osd_window", num_det=0, **kwargs):
    """Host only (needs no device): the forms a decoder built now would take -- ``last_form`` of that decoder before its first
    launch (``kind``, ``stream_serial`` and ``depth_launch`` are -1).  ``windows``: a ``windows.WindowPlan`` (a
    ``SlidingWindowDecoder``), or a list of ``(matrix, channel_probs)`` / ``(matrix, channel_probs, row0, col0, commit)`` with
    ``num_det`` rows in the global check matrix (0: one window, as ``osd_window`` / ``bpgdg_decoder`` / ``bpgd_decoder`` take it).
    ``decoder`` and the keyword arguments are those of the decoder.  A plan no window kernel takes reports ``general=1``; input no form
    takes (a matrix with an empty row, an OSD order out of range) raises ValueError."""
    if hasattr(windows, "windows"):
        num_det = windows.chk.shape[0]
        windows = [(w.mat, w.prior, w.row0, w.col0, w.commit) for w in windows.windows]
    if decoder == "osd_window":
        method, order = _parse_osd_method(kwargs.get("osd_method", "osd_0"), kwargs.get("osd_order", 0))
        new_n = kwargs.get("new_n", None)
        p = _lib.OsdwParams(int(kwargs.get("pre_max_iter", 8)), int(kwargs.get("post_max_iter", 100)),
                            float(kwargs.get("ms_scaling_factor", 1.0)), int(new_n) if new_n else 0, method, order)
        pp, gp = C.byref(p), None
    elif decoder in ("bpgdg_decoder", "bpgd_decoder", "bp_history_decoder"):
        p = _gdg_params(kwargs, {"bpgdg_decoder": 0, "bpgd_decoder": 1, "bp_history_decoder": 2}[decoder])
        pp, gp = None, C.byref(p)
    else:
        raise ValueError(f"unknown window decoder {decoder!r}")
    keep = []
    descs = (_lib.WindowDesc * len(windows))()
    for i, w in enumerate(windows):
        c = _Csr(w[0], w[1])
        keep.append(c)
        descs[i].graph = c.desc
        if len(w) > 2:
            descs[i].row0, descs[i].col0, descs[i].commit = int(w[2]), int(w[3]), int(w[4])
    plan = np.zeros(_lib.FORM_PLAN_WORDS, np.int32)
    wins = np.full((len(windows), _lib.FORM_WINDOW_WORDS), -1, np.int32)
    if _lib.lib().swd_window_forms(len(windows), C.cast(descs, C.c_void_p), int(num_det), pp, gp, plan.ctypes.data, wins.ctypes.data):
        raise ValueError(f"swd_window_forms failed: {_lib.last_error()}")
    return _form_dict(plan, wins)


def diag_libm(op, x, y=None, device=0):
    """Diagnostics (include/swd.h swd_diag_libm): one routine of the quaternary decoder's arithmetic on the device, element by
    element.  ``op``: 0 exp, 1 exp with its table in LDS, 2 log1p, 3 log1pexp, 4 logaddexp(x, y), 5 / 6 the general form's copies of
    3 / 4.  ``x`` (and ``y`` for ops 4 and 6): float64 numpy arrays -- copied to ``device`` and back, a numpy array returns -- or
    contiguous float64 CUDA tensors, evaluated on their device and the current stream, a tensor returns."""
    import torch
    host = not isinstance(x, torch.Tensor)
    binary = op in (4, 6)
    if binary and y is None:
        raise ValueError("ops 4 and 6 take x and y")
    if host:
        dev = torch.device("cuda", int(device))
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
        yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev) if binary else None
    else:
        xt, yt = x, (y if binary else None)
    for t in (xt, yt):
        if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.shape != xt.shape or t.device != xt.device):
            raise ValueError("x and y must be contiguous float64 CUDA tensors of one shape on one device")
    out = torch.empty_like(xt)
    rc = _lib.lib().swd_diag_libm(xt.device.index, int(op), xt.numel(), xt.data_ptr(), yt.data_ptr() if binary else None, out.data_ptr(),
                                  torch.cuda.current_stream(xt.device).cuda_stream)
    if rc:
        raise ValueError(f"swd_diag_libm failed: {_lib.last_error()}")
    return out.cpu().numpy() if host else out


class bp_history_decoder(_Handle):
    """Plain min-sum BP with a 4-deep posterior history (reference: src/bp_guessing_decoder.pyx:5-158)
    and base class of the guessing decoders.  ``bpgdg_decoder``: the side branches of a shot's decimation tree run
    concurrently on different workgroups; with ``multi_thread=False`` (default) the result is that of the reference's
    deterministic single-thread ``gdg()`` bit for bit; ``multi_thread=True`` runs the reference's threaded ensemble
    (bpgd.cpp:419-688: main thread, 2^D - 1 tree threads, S - D side threads) with the thread bodies in a fixed order, equal to
    the reference on every syndrome whose winning path metric is unique (``last_stats[:, 7]`` counts the tied, different
    vectors) -- the hypotheses are the leaves of a prefix tree whose shared BP blocks and scans run once (gdg_ensemble_tree).
    Every decode of the ensemble has the state of a NEWLY BUILT reference object: when ``BPGD::reset`` fails the zero vector is
    returned (a re-used reference object returns its previous decode's ``min_pm_error``, bpgd.cpp:583, 619-625), and each thread's
    posterior history starts from zeros (a re-used reference thread keeps its own stale slots when ``max_iter_per_step < 4``);
    ``hypotheses=H`` is this package's own ensemble over every leaf of gdg()'s tree with H leaves (no reference counterpart)."""
    _mode, _destroy = 2, "swd_gdg_destroy"

    def __init__(self, parity_check_matrix, **kwargs):
        L = _lib.lib()
        self._csr = _Csr(parity_check_matrix, kwargs.get("channel_probs"))
        self.m, self.n = self._csr.m, self._csr.n
        self.device = int(kwargs.get("device", 0))
        p = _gdg_params(kwargs, self._mode)
        self._h = L.swd_gdg_create(C.byref(self._csr.desc), C.byref(p), self.device)
        if not self._h:
            raise _lib.error("swd_gdg_create")
        self._hist = np.zeros((4, self.n), dtype=np.float64)
        self._last = dict(status=0, iters=0, min_pm=0.0)

    def decode(self, input_vector):
        s = _as_synd(input_vector, self.m)
        out = np.zeros(self.n, dtype=np.uint8)
        st = np.zeros(_lib.STAT_WORDS, np.int32)
        pm = np.zeros(1, np.float64)
        rc = _lib.lib().swd_gdg_decode_batch(self._h, 1, s.ctypes.data, out.ctypes.data, st.ctypes.data,
                                             pm.ctypes.data, None, 0)
        if rc:
            raise _lib.error("swd_gdg_decode_batch")
        self._last = dict(status=int(st[0]), iters=int(st[1]), min_pm=float(pm[0]))
        return out.astype(np.int64)

    def decode_batch(self, syndromes):
        s = np.asarray(syndromes)
        if s.ndim != 2 or s.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape [B, {self.m}]")
        s = np.ascontiguousarray((s.astype(np.int64) & 0xFF).astype(np.uint8))
        B = s.shape[0]
        out = np.zeros((B, self.n), dtype=np.uint8)
        st = np.zeros((B, _lib.STAT_WORDS), np.int32)
        pm = np.zeros(B, np.float64)
        rc = _lib.lib().swd_gdg_decode_batch(self._h, B, s.ctypes.data, out.ctypes.data, st.ctypes.data,
                                             pm.ctypes.data, None, 0)
        if rc:
            raise _lib.error("swd_gdg_decode_batch")
        self.last_stats, self.last_min_pm = st, pm
        self.last_status = st[:, 0].copy()
        return out

    @property
    def last_form(self):
        """As ``osd_window.last_form`` (include/swd.h, swd_gdg_last_form)."""
        return _last_form("swd_gdg_last_form", self._h, 1)

    @property
    def converge(self):
        return bool(self._last["status"] & STATUS_CONVERGE)


class bpgdg_decoder(bp_history_decoder):
    """BP + guided decimation guessing (reference: src/bp_guessing_decoder.pyx:160-442).

    ``multi_thread=True`` and ``decode()`` one syndrome at a time: the reference keeps ONE ``BPGD_main_thread`` for the object's
    lifetime (bp_guessing_decoder.pyx:238-251) whose ``min_pm_error`` -- a vector over the POSITIONS of the sorted order, not over
    columns -- is never cleared (bpgd.cpp:597-599); when ``BPGD::reset`` fails, ``do_work`` returns before anything is written to it
    (:619-625) and the decoder copies the PREVIOUS decode's position vector over this decode's first new_n sorted columns.  The
    object reproduces that (``reuse_object=True``, the default; round 6): the device decodes with the state of a new object, the
    sorted order of the decode is recomputed from the pre-processing history it returns (stable argsort of the slot-order sum,
    bp_guessing_decoder.pyx:240-244), and the position vector is kept between calls.  ``decode_batch`` gives every shot a new
    object's state (zero vector on a failed reset)."""
    _mode = 0

    def __init__(self, parity_check_matrix, **kwargs):
        super().__init__(parity_check_matrix, **kwargs)
        nn = kwargs.get("new_n", None)
        self._new_n = min(int(nn), self.n) if nn else min(self.n, 2 * self.m)  # bp_guessing_decoder.pyx:186-189
        self._ens = kwargs.get("multi_thread", False) is True or kwargs.get("multi_thread", False) == 1
        self._ens = bool(self._ens) and "hypotheses" not in kwargs
        self._reuse = bool(kwargs.get("reuse_object", True))
        self._prev_pos = np.zeros(self._new_n, np.uint8)  # min_pm_error of a new object: zeros

    def decode(self, input_vector):
        if not (self._ens and self._reuse):
            return super().decode(input_vector)
        s = _as_synd(input_vector, self.m)
        out = np.zeros(self.n, dtype=np.uint8)
        st = np.zeros(_lib.STAT_WORDS, np.int32)
        pm = np.zeros(1, np.float64)
        hist = np.zeros((4, self.n), np.float64)
        rc = _lib.lib().swd_gdg_decode_batch(self._h, 1, s.ctypes.data, out.ctypes.data, st.ctypes.data, pm.ctypes.data, hist.ctypes.data, 0)
        if rc:
            raise _lib.error("swd_gdg_decode_batch")
        self._last = dict(status=int(st[0]), iters=int(st[1]), min_pm=float(pm[0]))
        exit_class = int(st[0]) & 0xFF
        if exit_class == EXIT_PRE:  # the pre-processing BP converged: the ensemble object is not touched
            return out.astype(np.int64)
        llr_sum = ((hist[0] + hist[1]) + hist[2]) + hist[3]
        cols = np.argsort(llr_sum, kind="stable")[:self._new_n]
        if exit_class == EXIT_FAIL_PEEL:  # BPGD::reset failed: the previous decode's position vector over THIS decode's sorted columns
            out[:] = 0
            out[cols] = self._prev_pos
        else:
            self._prev_pos = out[cols].copy()
        return out.astype(np.int64)


class bpgd_decoder(bp_history_decoder):
    """BP + guided decimation (reference: src/bp_guessing_decoder.pyx:473-571)."""
    _mode = 1


class bp4_osd(_Handle):
    """Quaternary BP + OSD (reference: src/bp4_osd.pyx).  ``decode(sx, sz)`` returns the int64 array of
    shape (2, n) the reference returns (row 0: X string, row 1: Z string).

    Columns of Hx / Hz have weight <= 10, except for up to 8 HEAVY columns (weight above 10 in Hx or in Hz, at any position, of
    any weight): the last qubit of the cycle-assembled and EG codes of Misc.ipynb cells 6-8, H = (H1 | 1), touches every check.
    Without ``general_osd=True`` (below) such a graph takes ``osd_order=-1`` only (``ValueError`` otherwise): ``camel_decode``
    never runs OSD, and ``decode`` returns the BP decisions of a shot that did not converge.  With ``osd_method="osd0"`` -- cell
    8's spelling -- the reference resets the order to 0; on a graph with heavy columns the caller's -1 then stands.
    ``heavy_columns`` reports what the decoder found.

    ``general_form=True`` (default False) takes a graph beyond those bounds -- every column above weight 10 (the EG codes
    [[273,111,17]] and [[1057,571,33]] of cell 8), more than 1024 checks, rows of any weight, more messages than 160 KB of LDS hold:
    one 1024-thread workgroup per shot with every array in HBM, the same results bit for bit.  It runs BP only, so like a graph with
    heavy columns it takes ``osd_order=-1`` (``ValueError`` otherwise) and ``camel_decode``; any graph is taken, one the tuned
    kernels would take included.  Up to 1 048 576 qubits, 1 048 576 checks per matrix, 67 108 864 edges in all.

    ``general_osd=True`` (default False) lifts both ``osd_order=-1`` restrictions: the shots BP leaves unconverged are finished by
    an elimination kernel that keeps its arrays in HBM (one 1024-thread workgroup per shot, no bound on a column's weight), on a
    graph with heavy columns behind the tuned BP kernel, with ``general_form=True`` beside it behind the general one, and on any
    other graph too (in place of the tuned elimination kernel) -- OSD-0, ``osd_e`` and ``osd_cs`` with the reference's results bit
    for bit.  ``osd_method="osd0"`` then resets the order to 0 as the reference does, so cell 8's ``("osd0", -1)`` runs OSD-0
    inside ``decode``; ``osd_order=-1`` with the other methods stays "no OSD".  Bounds (``ValueError``): at most 4096 checks per
    matrix, and one shot's elimination arrays within 8 GiB.  ``rank_x`` / ``rank_z`` are the host GF(2) ranks."""
    _destroy = "swd_bp4_destroy"

    def __init__(self, Hx, Hz, **kwargs):
        L = _lib.lib()
        if not (isinstance(Hx, np.ndarray) or sp.issparse(Hx)):
            raise TypeError("The input matrix is of an invalid type. Please input a np.ndarray or "
                            "scipy.sparse.spmatrix object.")
        if Hx.shape[1] != Hz.shape[1]:
            raise ValueError("Hx, Hz blocklength does not match!")
        n = Hx.shape[1]
        probs = []
        for key in ("channel_probs_x", "channel_probs_y", "channel_probs_z"):
            v = kwargs.get(key)
            if v is None:
                raise ValueError(f"{key} is required")
            v = np.ascontiguousarray(v, dtype=np.float64)
            if len(v) != n:
                raise ValueError("The length of the channel probability vector must be eqaul to the "
                                 f"block length n={n}.")
            probs.append(v)
        self._px, self._py, self._pz = probs
        self._cx, self._cz = _Csr(Hx, self._px), _Csr(Hz, self._pz)
        self.mx, self.mz, self.n = self._cx.m, self._cz.m, n
        method, order = _parse_osd_method(kwargs.get("osd_method", "osd_0"), kwargs.get("osd_order", 0))
        self.device = int(kwargs.get("device", 0))
        asked = int(kwargs.get("osd_order", 0))
        if method == 0 and asked < 0:
            # (swd_bp4_create resets it to 0 like the reference, except on a graph with heavy columns or in the general form without
            # general_osd=True: include/swd.h)
            order = asked
        p = _lib.Bp4Params(int(kwargs.get("max_iter", 32)), float(kwargs.get("ms_scaling_factor", 1.0)), method, order)
        self._h = L.swd_bp4_create_ex(C.byref(self._cx.desc), C.byref(self._cz.desc), self._px.ctypes.data,
                                      self._py.ctypes.data, self._pz.ctypes.data, C.byref(p), self.device,
                                      (1 if kwargs.get("general_form", False) else 0) | (2 if kwargs.get("general_osd", False) else 0))
        if not self._h:
            raise _lib.error("swd_bp4_create")
        i = [C.c_int32() for _ in range(5)]
        L.swd_bp4_info(self._h, *[C.byref(x) for x in i])
        self.rank_x, self.rank_z = i[3].value, i[4].value
        self._last = dict(status=0, iters=0)
        self._lpr = np.zeros((3, n))
        self._osd0 = np.zeros((2, n), np.int64)
        self._out = np.zeros((2, n), np.int64)

    def decode_batch(self, synd_x, synd_z, return_llr=False, details=True):
        """[B, mx], [B, mz] -> uint8 [B, 2, n] (X string, Z string per decode).  ``details=False`` leaves the posteriors, the OSD-0
        vectors and the BP decisions on the device (``last_llr`` / ``last_osd0`` / ``last_bp_decoding`` become None): 2 n + 32 bytes
        come back per decode instead of 30 n."""
        sx, sz = np.asarray(synd_x), np.asarray(synd_z)
        if sx.ndim != 2 or sx.shape[1] != self.mx or sz.ndim != 2 or sz.shape[1] != self.mz or sx.shape[0] != sz.shape[0]:
            raise ValueError(f"syndromes must have shapes [B, {self.mx}] and [B, {self.mz}]")
        sx = np.ascontiguousarray((sx.astype(np.int64) & 0xFF).astype(np.uint8))
        sz = np.ascontiguousarray((sz.astype(np.int64) & 0xFF).astype(np.uint8))
        B = sx.shape[0]
        out = np.zeros((B, 2, self.n), np.uint8)
        st = np.zeros((B, _lib.STAT_WORDS), np.int32)
        lpr = np.zeros((B, 3, self.n)) if details else None
        osd0 = np.zeros((B, 2, self.n), np.uint8) if details else None
        bpd = np.zeros((B, 2, self.n), np.uint8) if details else None
        rc = _lib.lib().swd_bp4_decode_batch(self._h, B, sx.ctypes.data, sz.ctypes.data, out.ctypes.data, st.ctypes.data,
                                             lpr.ctypes.data if details else None, osd0.ctypes.data if details else None,
                                             bpd.ctypes.data if details else None)
        if rc:
            raise _lib.error("swd_bp4_decode_batch")
        self.last_stats, self.last_status, self.last_iterations = st, st[:, 0].copy(), st[:, 1].copy()
        self.last_llr, self.last_osd0, self.last_bp_decoding = lpr, osd0, bpd
        return out

    def decode_batch_device(self, synd_x, synd_z, out=None, stats=None, llr=None, stream=None):
        """Device-resident batch: ``synd_x`` [B, mx], ``synd_z`` [B, mz] contiguous torch uint8 CUDA tensors ->
        (out uint8 [B, 2, n], stats int32 [B, 8]); ``llr`` (float64 [B, 3, n], optional) receives the posterior LLRs.
        Asynchronous on the current (or given) torch stream."""
        import torch
        B, dev = synd_x.shape[0], synd_x.device
        for t, m in ((synd_x, self.mx), (synd_z, self.mz)):
            if t.dtype != torch.uint8 or t.dim() != 2 or t.shape != (B, m) or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"syndromes must be contiguous uint8 CUDA tensors [B, {self.mx}] and [B, {self.mz}]")
        out = torch.empty((B, 2, self.n), dtype=torch.uint8, device=dev) if out is None else out
        stats = torch.empty((B, _lib.STAT_WORDS), dtype=torch.int32, device=dev) if stats is None else stats
        st = torch.cuda.current_stream(dev) if stream is None else stream
        rc = _lib.lib().swd_bp4_decode_batch_dev(self._h, B, synd_x.data_ptr(), synd_z.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                                 llr.data_ptr() if llr is not None else None, None, None, st.cuda_stream)
        if rc:
            raise _lib.error("swd_bp4_decode_batch_dev")
        return out, stats

    @property
    def general_form(self):
        """True when the decoder runs the general form (``general_form=True`` at construction; include/swd.h swd_bp4_is_general)."""
        return _lib.lib().swd_bp4_is_general(self._h) == 1

    @property
    def general_osd(self):
        """True when the decoder was created with ``general_osd=True``: its OSD runs in the general elimination kernel
        (include/swd.h swd_bp4_is_general_osd)."""
        return _lib.lib().swd_bp4_is_general_osd(self._h) == 1

    @property
    def heavy_columns(self):
        """(count, largest weight) of the columns the decoder treats as heavy (include/swd.h swd_bp4_heavy_info); (0, 0) for a
        graph within the column-weight bound, which takes the kernel forms ``last_form`` reports, and in the general form, where
        no column is special."""
        c, d = C.c_int32(), C.c_int32()
        if _lib.lib().swd_bp4_heavy_info(self._h, C.byref(c), C.byref(d)):
            raise _lib.error("swd_bp4_heavy_info")
        return c.value, d.value

    @property
    def last_form(self):
        """The form of the BP kernel the most recent launch took (include/swd.h swd_bp4_last_form): dict with split, lazy, fast,
        wmax, dm, threads, skew, overlapped; None before the first launch."""
        keys = ("split", "lazy", "fast", "wmax", "dm", "threads", "skew", "overlapped")
        v = [C.c_int32() for _ in keys]
        if _lib.lib().swd_bp4_last_form(self._h, *[C.byref(x) for x in v]):
            return None
        return {k: x.value for k, x in zip(keys, v)}

    def decode(self, input_vector_x, input_vector_z):
        sx, sz = np.asarray(input_vector_x), np.asarray(input_vector_z)
        if sx.shape[0] != self.mx or sz.shape[0] != self.mz:
            raise ValueError(f"The input to the bp4_osd.decode must be a syndrome (of length={self.mx}).")
        out = self.decode_batch(sx[None, :], sz[None, :])
        self._last = dict(status=int(self.last_status[0]), iters=int(self.last_iterations[0]))
        self._lpr = self.last_llr[0]
        self._out = out[0].astype(np.int64)
        self._bp = self.last_bp_decoding[0].astype(np.int64)
        if (self._last["status"] & 0xFF) in (EXIT_PRE, EXIT_OSD):
            self._osd0 = self.last_osd0[0].astype(np.int64)
        if (self._last["status"] & 0xFF) == EXIT_OSD:  # osdw_decoding_* only change when the OSD ran (bp4_osd.pyx:217-219)
            self._osdw = self._out.copy()
        return self._out.copy()

    def camel_decode_batch(self, synd_x, synd_z):
        """camel_decode (bp4_osd.pyx:223-247) for a batch: uint8 [B, 2, n]; ``last_status`` / ``last_iterations`` /
        ``last_min_pm`` per shot.  Every shot sees a newly built object: zero vectors when no run converges."""
        sx, sz = np.asarray(synd_x), np.asarray(synd_z)
        if sx.ndim != 2 or sx.shape[1] != self.mx or sz.ndim != 2 or sz.shape[1] != self.mz or sx.shape[0] != sz.shape[0]:
            raise ValueError(f"syndromes must have shapes [B, {self.mx}] and [B, {self.mz}]")
        sx = np.ascontiguousarray((sx.astype(np.int64) & 0xFF).astype(np.uint8))
        sz = np.ascontiguousarray((sz.astype(np.int64) & 0xFF).astype(np.uint8))
        B = sx.shape[0]
        out = np.zeros((B, 2, self.n), np.uint8)
        st = np.zeros((B, _lib.STAT_WORDS), np.int32)
        pm = np.full(B, 10000.0)
        rc = _lib.lib().swd_bp4_camel_decode_batch(self._h, B, sx.ctypes.data, sz.ctypes.data, out.ctypes.data, st.ctypes.data,
                                                   pm.ctypes.data)
        if rc:
            raise _lib.error("swd_bp4_camel_decode_batch")
        self.last_stats, self.last_status, self.last_iterations, self.last_min_pm = st, st[:, 0].copy(), st[:, 1].copy(), pm
        return out

    def camel_decode(self, input_vector_x, input_vector_z):
        """Same call as the reference's ``camel_decode``; the returned (2, n) array is also what
        ``osd0_decoding_x`` / ``osd0_decoding_z`` hold afterwards."""
        sx, sz = np.asarray(input_vector_x), np.asarray(input_vector_z)
        if sx.shape[0] != self.mx or sz.shape[0] != self.mz:
            raise ValueError(f"The input to the bp4_osd.decode must be a syndrome (of length={self.mx}).")
        out = self.camel_decode_batch(sx[None, :], sz[None, :])
        self._last = dict(status=int(self.last_status[0]), iters=int(self.last_iterations[0]))
        self._min_pm = float(self.last_min_pm[0])
        self._osd0 = out[0].astype(np.int64)
        return self._osd0.copy()

    converge = property(lambda self: 1 if (self._last["status"] & STATUS_CONVERGE) else 0)
    bp_iteration = property(lambda self: self._last["iters"])
    min_pm = property(lambda self: getattr(self, "_min_pm", 0.0))
    bp_decoding_x = property(lambda self: getattr(self, "_bp", np.zeros((2, self.n), np.int64))[0].copy())
    bp_decoding_z = property(lambda self: getattr(self, "_bp", np.zeros((2, self.n), np.int64))[1].copy())
    osdw_decoding_x = property(lambda self: getattr(self, "_osdw", np.zeros((2, self.n), np.int64))[0].copy())
    osdw_decoding_z = property(lambda self: getattr(self, "_osdw", np.zeros((2, self.n), np.int64))[1].copy())
    osd0_decoding_x = property(lambda self: self._osd0[0].copy())
    osd0_decoding_z = property(lambda self: self._osd0[1].copy())

    @property
    def log_prob_ratios(self):
        return np.ascontiguousarray(self._lpr.T)


class _HostPool:
    """Result arrays of the host-buffer calls, recycled.  A fresh ``np.empty`` of 36 MB (total_e_hat of a 4096-shot batch of the
    [[144,12,12]] experiment) is 9 000 untouched pages that the unpacking threads fault in one by one -- a quarter of the call.  The
    arrays handed out are views of pooled base arrays; a base whose views have all been dropped by the caller (reference count back
    at the pool's own) is handed out again, warm.  A caller that keeps every result simply gets fresh arrays as before."""

    def __init__(self, per_shape=3, shapes=6):
        self._bufs, self._per_shape, self._shapes = {}, per_shape, shapes
        # What sys.getrefcount reports for a pooled base nobody else holds depends on the interpreter (borrowed operand-stack
        # references, free-threaded builds): measure it with the loop shape take() uses instead of assuming CPython 3.10's 3, and
        # check the probe the other way -- one live view must read exactly one more.  A probe that disagrees switches recycling off.
        self._idle = self._probe(hold_view=False)
        if self._idle is None or self._probe(hold_view=True) != self._idle + 1:
            self._idle = None

    @staticmethod
    def _probe(hold_view):
        import sys
        lst = [np.empty(4, np.uint8)]
        view = lst[0][...] if hold_view else None
        n = None
        for base in lst:
            n = sys.getrefcount(base)
        del view
        return n

    def take(self, shape, dtype):
        import sys
        key = (tuple(int(x) for x in shape), np.dtype(dtype).str)
        if self._idle is None:  # reference counts are not readable the way the probe expects: plain fresh arrays
            return np.empty(key[0], dtype)
        lst = self._bufs.get(key)
        if lst is None:
            if len(self._bufs) >= self._shapes:
                self._bufs.pop(next(iter(self._bufs)))
            lst = self._bufs[key] = []
        for base in lst:
            if sys.getrefcount(base) == self._idle:  # the calibrated count of a base with no view alive
                return base[...]
        base = np.empty(key[0], dtype)
        if len(lst) < self._per_shape:
            lst.append(base)
        return base[...]


class SlidingWindowDecoder(_Handle):
    """The (W,F) sliding-window loop of the reference harness (/root/reference/osd.py:130-179) for
    a whole batch of shots in ONE launch: a workgroup carries a shot through all its windows,
    committing ``commit`` columns per window and folding them back into the residual syndrome.

    ``plan`` is a ``windows.WindowPlan``; decoder kwargs are those of ``osd_window`` and apply to
    every window like in osd.py:152-161.

    ``window_loop`` says who runs the loop over the windows (read back as the attribute ``window_loop``: "pipeline", "host" or
    "device"; ``distinct_windows`` is the number of different window graphs of the plan):
      None      the one-launch pipeline; if the plan is beyond its kernels (the library refuses it with SWD_ERR_CAPACITY), the
                host loop -- one batched device decode per window through host memory, commit and residual syndrome on the host,
                ``decode()`` only;
      "host"    that host loop on any plan (it records every statistics word of a window decode; the fall-back of ``None``
                keeps to words 0 and 1 for ``osd_window``, as it always did);
      "device"  the device window loop on any plan (C ABI: swd_window_loop_*, csrc/swd_loop.hip): one single-window decoder per
                distinct window, residual syndrome, commit and accounting on the device, nothing synchronised on the host.  It
                serves ``decode``, ``decode_device`` and ``MemoryExperiment``; stream objects, sessions and rolling experiments
                need the one-launch pipeline."""
    _destroy = "swd_pipeline_destroy"

    def __init__(self, plan, device=0, decoder="osd_window", window_loop=None, **kwargs):
        if window_loop not in (None, "host", "device"):
            raise ValueError(f"window_loop must be None, 'host' or 'device', not {window_loop!r}")
        L = _lib.lib()
        self.plan = plan
        self.W = len(plan.windows)
        self.num_det, self.num_col = plan.chk.shape
        self.decoder = decoder
        if decoder == "osd_window":
            method, order = _parse_osd_method(kwargs.get("osd_method", "osd_0"), kwargs.get("osd_order", 0))
            new_n = kwargs.get("new_n", None)
            p = _lib.OsdwParams(int(kwargs.get("pre_max_iter", 8)), int(kwargs.get("post_max_iter", 100)),
                                float(kwargs.get("ms_scaling_factor", 1.0)), int(new_n) if new_n else 0, method, order)
        elif decoder in ("bpgdg_decoder", "bpgd_decoder", "bp_history_decoder"):
            p = _gdg_params(kwargs, {"bpgdg_decoder": 0, "bpgd_decoder": 1, "bp_history_decoder": 2}[decoder])
        else:
            raise ValueError(f"unknown window decoder {decoder!r}")
        self._keep = []
        descs = (_lib.WindowDesc * self.W)()
        for i, w in enumerate(plan.windows):
            c = _Csr(w.mat, w.prior)
            self._keep.append(c)
            descs[i].graph = c.desc
            descs[i].row0, descs[i].col0, descs[i].commit = int(w.row0), int(w.col0), int(w.commit)
        chk = _Csr(plan.chk, plan.priors)
        self._keep.append(chk)
        self.device = int(device)
        self._pool = _HostPool()
        self._loop = None
        self.num_obs = int(plan.obs.shape[0]) if plan.obs is not None else 0
        self.window_loop = "pipeline"
        if window_loop == "device":
            od = self._obs_desc() if 0 < self.num_obs <= 32 else None
            self._h = L.swd_window_loop_create(self.W, C.cast(descs, C.c_void_p), C.byref(chk.desc), C.byref(od) if od is not None else None,
                                               0 if decoder == "osd_window" else 1, C.cast(C.pointer(p), C.c_void_p), self.device)
            if not self._h:
                raise _lib.error("swd_window_loop_create")
            self._destroy, self.window_loop = "swd_window_loop_destroy", "device"
            k = C.c_int32()
            L.swd_window_loop_info(self._h, None, None, None, C.byref(k), None)
            self.distinct_windows = k.value
            self.lds_bytes, self.threads, self.node_pass = 0, 1024, "uniform"
            return
        from .windows import distinct_windows
        self.distinct_windows = len(set(distinct_windows(plan)))
        create = L.swd_pipeline_create if decoder == "osd_window" else L.swd_pipeline_create_gdg
        self._h = create(self.W, C.cast(descs, C.c_void_p), C.byref(chk.desc), C.byref(p), self.device) if window_loop is None else None
        if not self._h:
            if window_loop == "host" or _lib.last_error_class() == _lib.ERR_CAPACITY:
                # windows beyond every kernel variant (e.g. the un-windowed [[288,12,18]] model, 2736 x 26 208): the window loop of
                # /root/reference/osd.py:130-179 as the reference runs it -- one device decoder per window (the general forms,
                # csrc/swd_huge.hip and csrc/swd_huge_gdg.hip), the residual syndrome det ^ chk @ total_e_hat between windows
                # (osd.py:165, 178) on the host
                cls = {"osd_window": osd_window, "bpgdg_decoder": bpgdg_decoder, "bpgd_decoder": bpgd_decoder,
                       "bp_history_decoder": bp_history_decoder}[decoder]
                self._loop = [cls(w.mat, channel_probs=w.prior, device=self.device,
                                  **{k: v for k, v in kwargs.items() if k != "device"}) for w in plan.windows]
                self._chk_t = sp.csr_matrix(plan.chk.T.astype(np.int32))
                self.lds_bytes, self.threads, self.node_pass = 0, 1024, "uniform"
                self.window_loop, self._all_stats = "host", window_loop == "host"
                self._obs_t = sp.csr_matrix(plan.obs.T.astype(np.int32)) if self.num_obs else None
                return
            raise _lib.error("swd_pipeline_create")
        i = [C.c_int32() for _ in range(5)]
        L.swd_pipeline_info(self._h, *[C.byref(x) for x in i])
        self.lds_bytes, self.threads = i[3].value, i[4].value
        self.node_pass = "depth" if _node_depth(L, "swd_pipeline_node_depth", self._h) else "uniform"  # (as osd_window.node_pass)
        if 0 < self.num_obs <= 32:
            if L.swd_pipeline_set_observables(self._h, C.byref(self._obs_desc())):
                raise _lib.error("swd_pipeline_set_observables")

    def _obs_desc(self):
        a = sp.csr_matrix(self.plan.obs)
        a.sort_indices()
        rp, ci = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
        self._keep += [rp, ci]
        return _lib.GraphDesc(a.shape[0], a.shape[1], int(rp[-1]), rp.ctypes.data, ci.ctypes.data, None)

    @property
    def last_form(self):
        """As ``osd_window.last_form``, one entry of ``windows`` per window (include/swd.h, swd_pipeline_last_form); None when a
        window loop runs over single-window decoders, on the host or on the device."""
        return _last_form("swd_pipeline_last_form", self._h, self.W) if self.window_loop == "pipeline" else None

    def _check_det(self, det_data):
        d = np.asarray(det_data)
        if d.ndim != 2 or d.shape[1] != self.num_det:
            raise ValueError(f"det_data must have shape [B, {self.num_det}]")
        if d.dtype != np.uint8 or not d.flags.c_contiguous:
            d = np.ascontiguousarray((d.astype(np.int64) & 0xFF).astype(np.uint8))
        return d

    def decode(self, det_data, packed=False):
        """det_data [B, num_det] (host) -> total_e_hat uint8 [B, num_col]; per-window records in
        ``last_stats`` [B, W, 8] and ``last_min_pm`` [B, W].  ``packed=True`` returns total_e_hat bit-packed instead,
        uint8 [B, ceil(num_col / 8)] (``np.unpackbits(bits, axis=1, count=num_col, bitorder="little")`` gives the bytes): the
        faults always travel device -> host in that form (1098 B per shot instead of 8784 for the [[144,12,12]] experiment)."""
        d = self._check_det(det_data)
        B = d.shape[0]
        if self._loop is not None:
            return self._decode_window_loop(d, packed)
        pool = self._pool
        device_loop = self.window_loop == "device"  # (it returns bytes; they are packed here)
        total = pool.take((B, (self.num_col + 7) // 8 if packed and not device_loop else self.num_col), np.uint8)
        st = pool.take((B, self.W, _lib.STAT_WORDS), np.int32)
        pm = pool.take((B, self.W), np.float64)
        shot = np.zeros((B, 2), np.int32)
        name = "swd_window_loop_decode" if device_loop else "swd_pipeline_decode_packed" if packed else "swd_pipeline_decode"
        rc = getattr(_lib.lib(), name)(self._h, B, d.ctypes.data, total.ctypes.data, st.ctypes.data, pm.ctypes.data, shot.ctypes.data)
        if rc:
            raise _lib.error(name)
        self.last_stats, self.last_min_pm = st, pm
        self.last_obs_flips, self.last_flagged = shot[:, 0].astype(np.uint32), shot[:, 1].astype(bool)
        return np.packbits(total, axis=1, bitorder="little") if packed and device_loop else total

    def _decode_window_loop(self, d, packed):
        """the window loop for plans no pipeline kernel takes: per window one batched device decode, commit, residual"""
        B = d.shape[0]
        total = np.zeros((B, self.num_col), np.uint8)
        st = np.zeros((B, self.W, _lib.STAT_WORDS), np.int32)
        pm = np.zeros((B, self.W), np.float64)
        cur = d
        for wi, (w, dec) in enumerate(zip(self.plan.windows, self._loop)):
            out = dec.decode_batch(np.ascontiguousarray(cur[:, w.row0:w.row1])) if B else np.zeros((0, w.mat.shape[1]), np.uint8)
            total[:, w.col0:w.col0 + w.commit] = out[:, :w.commit]
            if B and self.decoder == "osd_window" and not self._all_stats:
                st[:, wi, 0], st[:, wi, 1], pm[:, wi] = dec.last_status, dec.last_iterations, dec.last_min_pm
            elif B:  # the guessing decoders: every statistics word of the window decode (include/swd.h)
                st[:, wi], pm[:, wi] = dec.last_stats, dec.last_min_pm
            cur = ((d.astype(np.int32) + (sp.csr_matrix(total) @ self._chk_t).toarray()) % 2).astype(np.uint8)  # osd.py:178
        self.last_stats, self.last_min_pm = st, pm
        self.last_flagged = cur.any(axis=1)
        flips = np.zeros(B, np.uint32)
        if self._obs_t is not None and self.num_obs <= 32 and B:
            bits = ((sp.csr_matrix(total) @ self._obs_t).toarray() % 2).astype(np.uint32)
            flips = (bits << np.arange(self.num_obs, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
        self.last_obs_flips = flips
        return np.packbits(total, axis=1, bitorder="little") if packed else total

    def _no_loop(self, what, device_ok=False):
        if self.window_loop == "device" and not device_ok:
            raise RuntimeError(f"{what} needs the one-launch pipeline; this decoder runs the device window loop of {self.decoder} decodes "
                               f"(window_loop=\"device\"), which serves decode(), decode_device() and MemoryExperiment")
        if self._loop is not None:
            raise RuntimeError(f"{what} needs the one-launch pipeline; this plan's windows are beyond every kernel variant and run as a "
                               f"window loop of {self.decoder} decodes (use decode(); window_loop=\"device\" runs that loop on the "
                               f"device and also serves decode_device() and MemoryExperiment)")

    def _no_device_loop(self, what):
        """the pipeline's own diagnostics: the device window loop's handle is no pipeline"""
        if self.window_loop == "device":
            self._no_loop(what)

    def stream(self, max_shots, packed=False, want_stats=True):
        """Streaming form for consecutive batches (``SlidingWindowStream``): two batches in flight on two lanes of this
        pipeline, copies and unpacking of batch k overlapped with the launch of batch k + 1."""
        self._no_loop("stream()")
        return SlidingWindowStream(self, max_shots, packed=packed, want_stats=want_stats)

    def session(self, max_shots):
        """Online form (``SlidingWindowSession``): the detector rows of a batch arrive in pieces, every window is decoded and
        committed as soon as its last row is there; results equal ``decode`` of the whole experiment."""
        self._no_loop("session()")
        return SlidingWindowSession(self, max_shots)

    def rolling_session(self, max_shots):
        """Rolling form (``RollingSession``): this decoder's plan of R0 rounds serves as a template (first, body and last window)
        for experiments of every length ``R = R0 (mod F)``, known only when they end; per-shot device state is one frame of
        residual rows, whatever R.  Results equal ``SlidingWindowDecoder(plan_windows(R)).decode``.  ValueError if the plan is
        not periodic between its first and its last window (``windows.rolling_template``)."""
        self._no_loop("rolling_session()")
        return RollingSession(self, max_shots)

    def measurement_session(self, max_shots, mmap):
        """Online form fed with the raw measurement record (``MeasurementSession``): ``mmap`` is the experiment's
        ``measurements.MeasurementMap``; a device front end turns the arriving bits into detector rows in front of ``session``'s
        merge, and ``finish`` returns the corrected logical readout.  ValueError if the map does not fit the plan."""
        return MeasurementSession(self, max_shots, mmap)

    def rolling_measurement_session(self, max_shots, mmap):
        """Rolling form fed with the raw measurement record (``RollingMeasurementSession``); ``mmap`` is the map of the template's
        own R0 rounds."""
        return RollingMeasurementSession(self, max_shots, mmap)

    def decode_stream(self, batches, packed=False, want_stats=True):
        """Generator over an iterable of host batches [B_k, num_det]: yields (total_e_hat, stats, min_pm, obs_flips, flagged) per
        batch, in order, keeping two batches in flight (the deployment form of the shots loop of /root/reference/osd.py:130-191)."""
        st, it = None, iter(batches)
        try:
            for d in it:
                d = self._check_det(d)
                if st is not None and d.shape[0] > st.max_shots:  # a larger batch than the lanes were sized for: drain, then re-create
                    while st.pending:
                        yield st.pop()
                    st.close()
                    st = None
                if st is None:
                    st = self.stream(d.shape[0], packed=packed, want_stats=want_stats)
                if st.pending == 2:
                    yield st.pop()
                st.push(d)
            while st is not None and st.pending:
                yield st.pop()
        finally:
            if st is not None:
                st.close()

    def decode_device(self, det, total=None, stats=None, min_pm=None, shot_result=None, stream=None,
                      want_stats=True, want_min_pm=True):
        """torch uint8 CUDA tensor [B, num_det] -> (total [B, num_col], stats [B, W, 8], min_pm [B, W]);
        asynchronous on the current torch stream.  ``shot_result`` (int32 [B, 2] CUDA tensor, optional)
        receives the predicted observable-flip mask and the flagged bit of every shot.
        ``min_pm=None`` alone does NOT mean "no path metrics" here (unlike ``push_device``): with ``want_stats`` a
        buffer is allocated and returned, as it always was.  ``want_min_pm=False`` (and no ``min_pm`` tensor) gives the
        launch no destination: None is returned in its place, and the windows that leave through BP do not compute one."""
        import torch
        self._no_loop("decode_device()", device_ok=True)
        if det.dtype != torch.uint8 or det.dim() != 2 or det.shape[1] != self.num_det or det.stride(1) != 1:
            raise ValueError(f"det must be a uint8 tensor [B, {self.num_det}] with unit column stride")
        if not det.is_cuda or det.device.index != self.device:
            raise ValueError(f"det lives on {det.device}, the pipeline on cuda:{self.device}")
        if shot_result is not None and self.num_obs > 32:
            raise ValueError("shot_result carries at most 32 observables; decode the observables on the host for more")
        B, dev = det.shape[0], det.device
        for name, t in (("total", total), ("stats", stats), ("min_pm", min_pm), ("shot_result", shot_result)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} lives on {t.device}, the pipeline on cuda:{self.device}")
        total = torch.empty((B, self.num_col), dtype=torch.uint8, device=dev) if total is None else total
        if want_stats:
            stats = torch.empty((B, self.W, _lib.STAT_WORDS), dtype=torch.int32, device=dev) if stats is None else stats
            if want_min_pm:
                min_pm = torch.empty((B, self.W), dtype=torch.float64, device=dev) if min_pm is None else min_pm
        st = torch.cuda.current_stream(dev) if stream is None else stream
        name = "swd_window_loop_decode_dev" if self.window_loop == "device" else "swd_pipeline_decode_dev"
        rc = getattr(_lib.lib(), name)(self._h, B, det.data_ptr(), det.stride(0), total.data_ptr(),
                                       total.stride(0), stats.data_ptr() if stats is not None else None,
                                       min_pm.data_ptr() if min_pm is not None else None,
                                       shot_result.data_ptr() if shot_result is not None else None,
                                       st.cuda_stream)
        if rc:
            raise _lib.error(name)
        return total, stats, min_pm

    def check_status(self):
        """Synchronises the device and raises if any launch of this pipeline since the last check recorded a
        scheduling fault (a window whose predecessor never finished: exit class 6 in ``stats``).  The host-buffer
        ``decode`` checks by itself; callers of the asynchronous ``decode_device`` call this after their launches."""
        if self.window_loop != "pipeline":  # (the single-window decoders of a window loop have no predecessor to wait for)
            return
        flags = C.c_uint32(0)
        if _lib.lib().swd_pipeline_status(self._h, C.byref(flags)):
            raise _lib.error("swd_pipeline_status")
        if flags.value:
            raise RuntimeError(f"sliding-window pipeline recorded a scheduling fault (flags 0x{flags.value:x})")

    def set_profiling(self, on=True):
        self._no_device_loop("set_profiling()")
        _lib.lib().swd_pipeline_set_profiling(self._h, 1 if on else 0)

    def get_profile(self, B):
        """[B, W, 8] int64 ticks (100 MHz) per phase of the last launch (diagnostics)."""
        self._no_device_loop("get_profile()")
        out = np.zeros((B, self.W, 8), np.int64)
        if _lib.lib().swd_pipeline_get_profile(self._h, B, out.ctypes.data):
            raise RuntimeError(_lib.last_error())
        return out

    def set_timing(self, on=True):
        self._no_device_loop("set_timing()")
        _lib.lib().swd_pipeline_set_timing(self._h, 1 if on else 0)

    def get_timing(self):
        self._no_device_loop("get_timing()")
        ms, k = C.c_double(), C.c_int64()
        _lib.lib().swd_pipeline_get_timing(self._h, C.byref(ms), C.byref(k))
        return ms.value, k.value


class SlidingWindowStream(_Handle):
    """Two-lane stream of a ``SlidingWindowDecoder`` (C ABI: swd_pipeline_stream_*).  Host form: ``push(det)`` returns at once,
    ``pop()`` waits for the oldest batch in flight -> (total_e_hat, stats, min_pm, obs_flips, flagged).  Device form:
    ``push_device`` launches on the next lane with the caller's CUDA tensors (keep one set of outputs per lane), ``wait()`` joins."""
    _destroy = "swd_pipeline_stream_destroy"

    def __init__(self, dec, max_shots, packed=False, want_stats=True):
        self.dec, self.packed, self.want_stats = dec, bool(packed), bool(want_stats)
        self.max_shots = int(max_shots)
        flags = (_lib.STREAM_PACKED if packed else 0) | (0 if want_stats else _lib.STREAM_NO_STATS)
        dec._no_device_loop("SlidingWindowStream")
        self._h = _lib.lib().swd_pipeline_stream_create(dec._h, self.max_shots, flags)
        if not self._h:
            raise _lib.error("swd_pipeline_stream_create")
        self._sizes = []

    close = _Handle._release

    @property
    def pending(self):
        return len(self._sizes)

    def push(self, det_data):
        d = self.dec._check_det(det_data)
        if _lib.lib().swd_pipeline_stream_push(self._h, d.shape[0], d.ctypes.data):
            raise _lib.error("swd_pipeline_stream_push")
        self._sizes.append(d.shape[0])  # (the library has copied the detector bytes into its page-locked block)

    def pop(self):
        if not self._sizes:
            raise RuntimeError("stream pop: no batch in flight")
        B, dec = self._sizes.pop(0), self.dec
        pool = dec._pool
        total = pool.take((B, (dec.num_col + 7) // 8 if self.packed else dec.num_col), np.uint8)
        st = pool.take((B, dec.W, _lib.STAT_WORDS), np.int32) if self.want_stats else None
        pm = pool.take((B, dec.W), np.float64) if self.want_stats else None
        shot = np.empty((B, 2), np.int32)
        rc = _lib.lib().swd_pipeline_stream_pop(self._h, total.ctypes.data, st.ctypes.data if st is not None else None,
                                                pm.ctypes.data if pm is not None else None, shot.ctypes.data)
        if rc != B:
            raise _lib.error("swd_pipeline_stream_pop")
        return total, st, pm, shot[:, 0].astype(np.uint32), shot[:, 1].astype(bool)

    def push_device(self, det, total, stats=None, min_pm=None, shot_result=None, after=None):
        """CUDA tensors as in ``SlidingWindowDecoder.decode_device``; ``after``: a torch stream whose work so far must precede
        the launch -- the producer of ``det`` and the last reader of this lane's output tensors (default: the current stream,
        also when that is PyTorch's default stream, whose handle is 0); ``after=False``: no dependency, the caller has
        synchronised inputs and outputs itself."""
        import torch
        dec = self.dec
        if det.dtype != torch.uint8 or det.dim() != 2 or det.shape[1] != dec.num_det or det.stride(1) != 1 or not det.is_cuda:
            raise ValueError(f"det must be a uint8 CUDA tensor [B, {dec.num_det}] with unit column stride")
        if after is False:
            aft = _lib.STREAM_NO_DEPENDENCY
        else:
            aft = (torch.cuda.current_stream(det.device) if after is None else after).cuda_stream or None  # 0 -> NULL = the legacy default stream
        rc = _lib.lib().swd_pipeline_stream_push_dev(self._h, det.shape[0], det.data_ptr(), det.stride(0), total.data_ptr(), total.stride(0),
                                                     stats.data_ptr() if stats is not None else None,
                                                     min_pm.data_ptr() if min_pm is not None else None,
                                                     shot_result.data_ptr() if shot_result is not None else None, aft)
        if rc:
            raise _lib.error("swd_pipeline_stream_push_dev")

    def wait(self, stream=None):
        """stream=None: the host waits for both lanes; a torch stream: that stream waits (device-side)."""
        if _lib.lib().swd_pipeline_stream_wait(self._h, stream.cuda_stream if stream is not None else None):
            raise _lib.error("swd_pipeline_stream_wait")

    def wait_last(self, stream):
        """the torch stream ``stream`` waits (device-side) for the lane of the most recent push alone: the batch on the other lane
        stays in flight.  RuntimeError if nothing has been pushed."""
        if _lib.lib().swd_pipeline_stream_wait_last(self._h, stream.cuda_stream or None):
            raise _lib.error("swd_pipeline_stream_wait_last")


class _SessionBase(_Handle):
    """What ``SlidingWindowSession`` and ``RollingSession`` share: the handle's life, ``begin`` and the checks of arriving rows.
    ``_C``: the prefix of the form's C symbols."""
    close = _Handle._release

    def begin(self, B):
        """Zero state for a batch of ``B <= max_shots`` shots; also restarts a session that has been used."""
        if getattr(_lib.lib(), self._C + "_begin")(self._h, int(B)):
            raise _lib.error(f"{self._C}_begin")
        self.B = int(B)

    def _host_rows(self, rows, name="det_rows"):
        """[B, k] host rows as a C-contiguous uint8 array"""
        d = np.asarray(rows)
        if d.ndim != 2 or d.shape[0] != self.B:
            raise ValueError(f"{name} must have shape [{self.B}, k]")
        if d.dtype != np.uint8 or not d.flags.c_contiguous:
            d = np.ascontiguousarray((d.astype(np.int64) & 0xFF).astype(np.uint8))
        return d

    def _check_device_rows(self, det_rows):
        import torch
        if det_rows.dtype != torch.uint8 or det_rows.dim() != 2 or det_rows.shape[0] != self.B or not det_rows.is_cuda or \
                (det_rows.shape[1] > 1 and det_rows.stride(1) != 1):
            raise ValueError(f"det_rows must be a uint8 CUDA tensor [{self.B}, k] with unit column stride")
        if det_rows.device.index != self.dec.device:
            raise ValueError(f"det_rows lives on {det_rows.device}, the pipeline on cuda:{self.dec.device}")


class SlidingWindowSession(_SessionBase):
    """Online session of a ``SlidingWindowDecoder`` (C ABI: swd_pipeline_session_*): the window loop of
    /root/reference/osd.py:130-179 driven by the arrival of detector rows.  The session keeps the residual syndrome,
    total_e_hat and the observable accumulators of one batch on the device; ``push`` takes the next rows of every shot (any
    number, in row order) and returns the windows they completed, each decoded on the rows received so far and committed --
    bit-identical to ``decode`` of the whole experiment, whatever the chunking."""
    _C, _destroy = "swd_pipeline_session", "swd_pipeline_session_destroy"

    def __init__(self, dec, max_shots):
        self.dec, self.max_shots, self.B = dec, int(max_shots), 0
        dec._no_device_loop("SlidingWindowSession")
        self._h = _lib.lib().swd_pipeline_session_create(dec._h, self.max_shots)
        if not self._h:
            raise _lib.error("swd_pipeline_session_create")

    def _progress(self):
        rows, done = C.c_int32(), C.c_int32()
        if _lib.lib().swd_pipeline_session_buffers(self._h, None, None, C.byref(rows), C.byref(done)):
            raise _lib.error("swd_pipeline_session_buffers")
        return rows.value, done.value

    @property
    def rows_received(self):
        return self._progress()[0]

    @property
    def windows_done(self):
        return self._progress()[1]

    @property
    def rows_needed(self):
        """Detector rows that must have arrived before the next window is decoded (``windows[next].row1``); None after the last."""
        done = self.windows_done
        return int(self.dec.plan.windows[done].row1) if done < self.dec.W else None

    def window(self, t):
        """(t, col0, faults [B, commit], stats [B, 8], min_pm [B]) of a committed window."""
        w, B = self.dec.plan.windows[t], self.B
        faults = np.empty((B, int(w.commit)), np.uint8)
        st, pm = np.empty((B, _lib.STAT_WORDS), np.int32), np.empty(B, np.float64)
        if _lib.lib().swd_pipeline_session_window(self._h, int(t), faults.ctypes.data, st.ctypes.data, pm.ctypes.data):
            raise _lib.error("swd_pipeline_session_window")
        return int(t), int(w.col0), faults, st, pm

    def push(self, det_rows):
        """det_rows [B, k] (host): the next k detector rows of every shot.  Returns the windows this call committed, in order, as
        ``(t, col0, faults [B, commit], stats [B, 8], min_pm [B])`` -- ``faults`` is ``total_e_hat[:, col0:col0 + commit]``."""
        d = self._host_rows(det_rows)
        first, count = C.c_int32(), C.c_int32()
        if _lib.lib().swd_pipeline_session_push(self._h, d.shape[1], d.ctypes.data, C.byref(first), C.byref(count)):
            raise _lib.error("swd_pipeline_session_push")
        return [self.window(t) for t in range(first.value, first.value + count.value)]

    def push_device(self, det_rows, stream=None):
        """torch uint8 CUDA tensor [B, k] with unit column stride (a column slice of a [B, num_det] tensor fits); merge, decode and
        commit are queued on ``stream`` (default: the current torch stream).  Returns (first, count) of the windows queued."""
        import torch
        self._check_device_rows(det_rows)
        st = torch.cuda.current_stream(det_rows.device) if stream is None else stream
        first, count = C.c_int32(), C.c_int32()
        k = det_rows.shape[1]
        if _lib.lib().swd_pipeline_session_push_dev(self._h, k, det_rows.data_ptr() if k else None, det_rows.stride(0) if k else 0,
                                                    C.byref(first), C.byref(count), st.cuda_stream):
            raise _lib.error("swd_pipeline_session_push_dev")
        return first.value, count.value

    def finish(self):
        """After the last window: (total_e_hat [B, num_col], stats [B, W, 8], min_pm [B, W], obs_flips [B], flagged [B]) as
        ``decode`` leaves them.  Before it: RuntimeError naming the rows still missing."""
        dec, B = self.dec, self.B
        total = np.empty((B, dec.num_col), np.uint8)
        st, pm = np.empty((B, dec.W, _lib.STAT_WORDS), np.int32), np.empty((B, dec.W), np.float64)
        shot = np.empty((B, 2), np.int32)
        if _lib.lib().swd_pipeline_session_finish(self._h, total.ctypes.data, st.ctypes.data, pm.ctypes.data, shot.ctypes.data):
            raise _lib.error("swd_pipeline_session_finish")
        return total, st, pm, shot[:, 0].astype(np.uint32), shot[:, 1].astype(bool)

    def total_device(self):
        """total_e_hat [B, num_col] of the batch as a torch CUDA tensor that ALIASES the session's buffer (columns committed so far,
        zeros elsewhere): for ``push_device`` callers, who order their reads after the stream they pushed on."""
        import torch
        ptr, stride = C.c_void_p(), C.c_int64()
        if _lib.lib().swd_pipeline_session_buffers(self._h, C.byref(ptr), C.byref(stride), None, None):
            raise _lib.error("swd_pipeline_session_buffers")

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": (self.B, self.dec.num_col), "typestr": "|u1", "data": (ptr.value, False), "version": 2,
                                      "strides": (stride.value, 1)}
        return torch.as_tensor(v, device=f"cuda:{self.dec.device}")


class RollingSession(_SessionBase):
    """Rolling session of a ``SlidingWindowDecoder`` (C ABI: swd_pipeline_rolling_*) whose plan of R0 rounds is the template: head =
    window 0, body = window 1, tail = last window.  It decodes experiments of any length ``R = R0 (mod F)`` rounds, known only when
    they end, with device memory that does not depend on R: per shot a frame of residual rows (``template.frame_rows``), an
    observable accumulator and a sticky flagged bit.  ``push`` takes the next detector rows of the SYNDROME rounds in pieces of any
    size and returns every window they completed; ``finish`` takes the rest and closes the experiment with the tail window.

    The final data-measurement block must go to ``finish``: ``push`` treats every block as a syndrome round and cannot tell the
    difference (a final block handed to ``push`` may complete a body window that the experiment does not have).

    Every result is bit-identical to ``SlidingWindowDecoder(plan_windows(R)).decode`` (windows.sliding_window_decode_rolling_host is
    the executable specification).  Per-window ``stats`` / ``min_pm`` come back with each step and are not retained.

    One thread at a time per session at this layer: ``push`` sizes its output arrays from a state query made before the call, so
    two threads pushing on one session would size them for the wrong state (the library then refuses the call, it does not
    overrun).  The C ABI itself may be called from any thread."""
    _C, _destroy = "swd_pipeline_rolling", "swd_pipeline_rolling_destroy"

    def __init__(self, dec, max_shots):
        from .windows import rolling_template
        self.template = rolling_template(dec.plan)  # ValueError names what is not periodic
        self.dec, self.max_shots, self.B = dec, int(max_shots), 0
        dec._no_device_loop("RollingSession")
        self._h = _lib.lib().swd_pipeline_rolling_create(dec._h, self.max_shots)
        if not self._h:
            raise _lib.error("swd_pipeline_rolling_create")
        info = (C.c_int32 * 8)()
        if _lib.lib().swd_pipeline_rolling_state(self._h, None, None, None, info, None):
            raise _lib.error("swd_pipeline_rolling_state")
        T = self.template
        self._need, self._cmax = int(info[1]), int(info[7])
        want = [T.frame_rows, T.head.row1, T.row_stride, T.tail.row1 - T.tail.row0, T.head.commit, T.body.commit, T.tail.commit,
                max(T.head.commit, T.body.commit)]
        if list(info) != [int(x) for x in want]:
            raise RuntimeError(f"rolling template: the library extracted {list(info)}, windows.rolling_template {want}")

    def _state(self):
        rows, done, fill, nbytes = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        if _lib.lib().swd_pipeline_rolling_state(self._h, C.byref(rows), C.byref(done), C.byref(fill), None, C.byref(nbytes)):
            raise _lib.error("swd_pipeline_rolling_state")
        return rows.value, done.value, fill.value, nbytes.value

    @property
    def rows_received(self):
        return self._state()[0]

    @property
    def rounds_received(self):
        """whole blocks of ``n_half`` rows received since ``begin``"""
        return self._state()[0] // self.template.n_half

    @property
    def windows_done(self):
        return self._state()[1]

    @property
    def rows_needed(self):
        """Rows still missing in the frame before ``push`` decodes the next head / body window."""
        return max(self._need - self._state()[2], 0)

    @property
    def device_bytes(self):
        """Bytes of device memory the session owns: a function of ``max_shots`` and the template, not of the rows received."""
        return self._state()[3]

    def _windows_for(self, k):
        have = self._state()[2] + int(k)
        return 0 if have < self._need else (have - self._need) // self.template.row_stride + 1

    def _commit(self, t):
        return int(self.template.head.commit if t == 0 else self.template.body.commit)

    def push(self, det_rows):
        """det_rows [B, k] (host): the next k rows of the syndrome rounds of every shot.  Returns the windows this call completed, in
        order, as ``(t, faults [B, commit_t], stats [B, 8], min_pm [B])``; ``t`` counts from 0 without bound."""
        d = self._host_rows(det_rows)
        n, B = self._windows_for(d.shape[1]) if self.B else 0, self.B
        faults = np.zeros((n, B, self._cmax), np.uint8)
        st, pm = np.empty((n, B, _lib.STAT_WORDS), np.int32), np.empty((n, B), np.float64)
        first, count = C.c_int64(), C.c_int32()
        if _lib.lib().swd_pipeline_rolling_push(self._h, d.shape[1], d.ctypes.data, n, faults.ctypes.data, st.ctypes.data, pm.ctypes.data,
                                                C.byref(first), C.byref(count)):
            raise _lib.error("swd_pipeline_rolling_push")
        return [(first.value + k, faults[k, :, :self._commit(first.value + k)], st[k], pm[k]) for k in range(count.value)]

    def push_device(self, det_rows, faults_out=None, stream=None):
        """torch uint8 CUDA tensor [B, k] with unit column stride; merge, decode and commit are queued on ``stream`` (default: the
        current torch stream).  ``faults_out``: optional contiguous uint8 CUDA tensor [n, B, commit_max] of the caller's, n >= the
        windows this call completes (``commit_max = max(head.commit, body.commit)``); window k of the call writes the first
        ``commit_t`` columns of ``faults_out[k]``.  Returns ``(t, faults, stats, min_pm)`` per window as CUDA tensors (views of
        ``faults_out``), valid once ``stream`` has reached them."""
        import torch
        self._check_device_rows(det_rows)
        st = torch.cuda.current_stream(det_rows.device) if stream is None else stream
        k, B, dev = det_rows.shape[1], self.B, det_rows.device
        n = self._windows_for(k) if self.B else 0
        with torch.cuda.stream(st):
            if faults_out is None:
                faults_out = torch.zeros((n, B, self._cmax), dtype=torch.uint8, device=dev)
            elif faults_out.dtype != torch.uint8 or faults_out.dim() != 3 or faults_out.shape[0] < n or not faults_out.is_contiguous() or \
                    tuple(faults_out.shape[1:]) != (B, self._cmax) or faults_out.device != dev:
                raise ValueError(f"faults_out must be a contiguous uint8 CUDA tensor [n >= {n}, {B}, {self._cmax}] on {dev}")
            stats = torch.empty((n, B, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
            pm = torch.empty((n, B), dtype=torch.float64, device=dev)
        first, count = C.c_int64(), C.c_int32()
        if _lib.lib().swd_pipeline_rolling_push_dev(self._h, k, det_rows.data_ptr() if k else None, det_rows.stride(0) if k else 0, n,
                                                    faults_out.data_ptr() if n else None, stats.data_ptr() if n else None,
                                                    pm.data_ptr() if n else None, C.byref(first), C.byref(count), st.cuda_stream):
            raise _lib.error("swd_pipeline_rolling_push_dev")
        return [(first.value + j, faults_out[j, :, :self._commit(first.value + j)], stats[j], pm[j]) for j in range(count.value)]

    def _check_finish(self, k):
        """ValueError unless the rows received plus ``k`` final rows make an experiment the template serves"""
        T = self.template
        rows, done, fill, _ = self._state()
        total, tail_rows = rows + k, T.tail.row1 - T.tail.row0
        if self.B and (k == 0 or done == 0 or fill + k != tail_rows):
            what = f"{total // T.n_half - 1} syndrome rounds" if total % T.n_half == 0 else "no whole number of rounds"
            why = "the final block must go to finish, not to push" if k == 0 else \
                ("fewer rows than the first and the last window need" if done == 0 else "not a length this template serves")
            raise ValueError(f"{total} detector rows ({rows} pushed, {k} final) make {what}: {why}; this template serves {T.lengths()}")

    def finish(self, final_rows):
        """final_rows [B, k] (host), k >= 1: the rest of the experiment, the final data-measurement block included.  The tail window
        is decoded and committed whole.  Returns ``(t, tail_faults [B, tail commit], stats [B, 8], min_pm [B], obs_flips [B],
        flagged [B])`` -- the last two as ``decode`` leaves ``last_obs_flips`` / ``last_flagged``.  ValueError, with the state
        untouched, if the rows do not make an experiment of ``R = R0 (mod F)`` rounds or are fewer than head and tail need."""
        d = self._host_rows(final_rows, "final_rows")
        self._check_finish(d.shape[1])
        B, t = self.B, self._state()[1]
        faults = np.empty((B, int(self.template.tail.commit)), np.uint8)
        st, pm, shot = np.empty((B, _lib.STAT_WORDS), np.int32), np.empty(B, np.float64), np.empty((B, 2), np.int32)
        if _lib.lib().swd_pipeline_rolling_finish(self._h, d.shape[1], d.ctypes.data, faults.ctypes.data, st.ctypes.data, pm.ctypes.data,
                                                  shot.ctypes.data):
            raise _lib.error("swd_pipeline_rolling_finish")
        return t, faults, st, pm, shot[:, 0].astype(np.uint32), shot[:, 1].astype(bool)

    def finish_device(self, final_rows, stream=None):
        """``finish`` with a CUDA tensor, queued on ``stream``: returns ``(t, tail_faults, stats, min_pm, obs_flips, flagged)`` as
        ``finish`` does, as CUDA tensors; ``obs_flips`` / ``flagged`` are the int32 columns of one [B, 2] tensor (bit mask; 0 or 1)."""
        import torch
        self._check_device_rows(final_rows)
        self._check_finish(final_rows.shape[1])
        st = torch.cuda.current_stream(final_rows.device) if stream is None else stream
        B, dev, t = self.B, final_rows.device, self._state()[1]
        with torch.cuda.stream(st):
            faults = torch.empty((B, int(self.template.tail.commit)), dtype=torch.uint8, device=dev)
            stats = torch.empty((B, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
            pm = torch.empty(B, dtype=torch.float64, device=dev)
            shot = torch.empty((B, 2), dtype=torch.int32, device=dev)
        if _lib.lib().swd_pipeline_rolling_finish_dev(self._h, final_rows.shape[1], final_rows.data_ptr(), final_rows.stride(0),
                                                      faults.data_ptr(), stats.data_ptr(), pm.data_ptr(), shot.data_ptr(), st.cuda_stream):
            raise _lib.error("swd_pipeline_rolling_finish_dev")
        return t, faults, stats, pm, shot[:, 0], shot[:, 1]


def _template_desc(a, keep):
    """CSR descriptor of a measurement template (no priors); the arrays are appended to ``keep``"""
    a = sp.csr_matrix(a)
    a.sort_indices()
    rp, ci = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
    keep += [rp, ci]
    return _lib.GraphDesc(a.shape[0], a.shape[1], int(rp[-1]), rp.ctypes.data, ci.ctypes.data, None)


class MeasurementFrontEnd(_Handle):
    """Detector front end (C ABI: swd_frontend_*): turns the raw measurement record of a batch of shots, arriving in pieces of any
    size, into detector rows on the device -- ``measurements.MeasurementMap.blocks(n_half)`` applied push by push.  Per shot it
    keeps the last complete round's outcomes and the bits of the round under way (``device_bytes`` depends on the map and
    ``max_shots`` only).  ``push`` / ``push_device`` take bits of the SYNDROME rounds and return the rows of the rounds they
    completed; ``finish`` / ``finish_device`` take the rest of the last syndrome round and the final block and return the remaining
    rows and the raw observable parities (uint32 masks).  ``packed=True``: bit ``i & 7`` of byte ``i >> 3`` of every chunk
    (``np.packbits(chunk, axis=1, bitorder="little")``)."""
    _destroy = "swd_frontend_destroy"
    close = _Handle._release

    def __init__(self, mmap, n_half, max_shots, device=0):
        blk = mmap.blocks(n_half)  # ValueError names what does not fit
        self.blocks, self.max_shots, self.device, self.B = blk, int(max_shots), int(device), 0
        self.n_half, self.meas_per_round, self.meas_final, self.num_obs = blk.n_half, blk.meas_per_round, blk.meas_final, blk.obs_tail.shape[0]
        # what the library refuses about the map and the batch is checked here: a failing create is then the device's
        if self.num_obs > 32:
            raise ValueError(f"at most 32 observables, the map has {self.num_obs}")
        if self.max_shots <= 0:
            raise ValueError("max_shots must be positive")
        if 2 * blk.meas_per_round + blk.meas_final > _lib.FRONTEND_STAGE_BYTES:
            raise ValueError(f"two rounds of {blk.meas_per_round} measurements and a final block of {blk.meas_final} exceed the "
                             f"{_lib.FRONTEND_STAGE_BYTES} bytes a launch of the front end stages")
        keep = []
        d = [_template_desc(t, keep) for t in (blk.head, blk.body, blk.tail, blk.obs_tail)]
        self._h = _lib.lib().swd_frontend_create(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), C.byref(d[3]) if self.num_obs else None,
                                                 blk.meas_per_round, blk.meas_final, blk.n_half, self.max_shots, self.device)
        if not self._h:
            raise _lib.error("swd_frontend_create")

    def begin(self, B):
        if _lib.lib().swd_frontend_begin(self._h, int(B)):
            raise _lib.error("swd_frontend_begin")
        self.B = int(B)

    def _state(self):
        bits, rounds, info, nbytes = C.c_int64(), C.c_int64(), (C.c_int32 * 8)(), C.c_int64()
        if _lib.lib().swd_frontend_state(self._h, C.byref(bits), C.byref(rounds), info, C.byref(nbytes)):
            raise _lib.error("swd_frontend_state")
        return bits.value, rounds.value, int(info[4]), bool(info[5]), nbytes.value

    @property
    def bits_received(self):
        return self._state()[0]

    @property
    def rounds_done(self):
        return self._state()[1]

    @property
    def device_bytes(self):
        return self._state()[4]

    def rows_for(self, nbits, final=False):
        """detector rows a push (``final``: the finish) of ``nbits`` bits completes; ValueError if a finish of that many bits does
        not complete the last syndrome round and bring the whole final block"""
        bits, rounds, fill, finished = self._state()[:4]
        nbits = int(nbits)
        if not final:
            return (fill + nbits) // self.meas_per_round * self.n_half
        pre = nbits - self.meas_final
        if self.B and (finished or pre < 0 or (fill + pre) % self.meas_per_round or rounds + (fill + pre) // self.meas_per_round < 1):
            raise ValueError(f"finish: {nbits} bits after {bits} received ({rounds} whole rounds of {self.meas_per_round}, {fill} bits of the "
                             f"next) do not complete the last syndrome round and bring the final block of {self.meas_final}")
        return ((fill + pre) // self.meas_per_round + 1) * self.n_half

    def _host_bits(self, meas, packed):
        """[B, k] host chunk -> (C-contiguous uint8 array, number of bits).  A packed chunk is [B, ceil(k / 8)] bytes and carries
        8 bits per byte unless ``packed`` is the bit count itself."""
        d = np.asarray(meas)
        if d.ndim != 2 or d.shape[0] != self.B:
            raise ValueError(f"meas must have shape [{self.B}, k]")
        if d.dtype != np.uint8:
            if _is_packed(packed):
                if ((d < 0) | (d > 255)).any():
                    raise ValueError("a packed chunk holds bytes: values 0..255")
                d = d.astype(np.uint8)
            else:
                d = (d != 0).astype(np.uint8)  # any non-zero value is a 1, as on the device
        return np.ascontiguousarray(d), _chunk_bits(d.shape[1], packed)

    def _check_device_bits(self, meas, packed):
        import torch
        if meas.dtype != torch.uint8 or meas.dim() != 2 or meas.shape[0] != self.B or not meas.is_cuda or (meas.shape[1] > 1 and meas.stride(1) != 1):
            raise ValueError(f"meas must be a uint8 CUDA tensor [{self.B}, k] with unit column stride")
        if meas.device.index != self.device:
            raise ValueError(f"meas lives on {meas.device}, the front end on cuda:{self.device}")
        return _chunk_bits(meas.shape[1], packed)

    def push(self, meas, packed=False):
        """meas [B, k] (host): the next bits of the syndrome rounds -> det_rows uint8 [B, rows completed]"""
        d, nbits = self._host_bits(meas, packed)
        rows = np.empty((self.B, self.rows_for(nbits) if self.B else 0), np.uint8)
        n = C.c_int32()
        if _lib.lib().swd_frontend_push(self._h, nbits, d.ctypes.data, _is_packed(packed), rows.ctypes.data, C.byref(n)):
            raise _lib.error("swd_frontend_push")
        assert n.value == rows.shape[1]
        return rows

    def finish(self, final_meas, packed=False):
        """final_meas [B, k] (host): the rest of the last syndrome round, then the final block -> (det_rows uint8 [B, rows],
        raw_obs uint32 [B]).  ValueError, with the state unchanged, if the bits do not end the experiment."""
        d, nbits = self._host_bits(final_meas, packed)
        rows = np.empty((self.B, self.rows_for(nbits, final=True) if self.B else 0), np.uint8)
        raw, n = np.zeros(self.B, np.uint32), C.c_int32()
        if _lib.lib().swd_frontend_finish(self._h, nbits, d.ctypes.data, _is_packed(packed), rows.ctypes.data, C.byref(n), raw.ctypes.data):
            raise _lib.error("swd_frontend_finish")
        return rows, raw

    def push_device(self, meas, packed=False, out=None, stream=None):
        """torch uint8 CUDA tensor [B, k] with unit column stride; one launch queued on ``stream`` (default: the current torch
        stream).  ``out``: optional uint8 CUDA tensor [B, >= rows] with unit column stride to write into.  -> det_rows [B, rows]."""
        import torch
        nbits = self._check_device_bits(meas, packed)
        st = torch.cuda.current_stream(meas.device) if stream is None else stream
        rows = self.rows_for(nbits) if self.B else 0
        if out is None:
            with torch.cuda.stream(st):
                out = torch.empty((self.B, rows), dtype=torch.uint8, device=meas.device)
        elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != self.B or out.shape[1] < rows or out.device != meas.device or \
                (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError(f"out must be a uint8 CUDA tensor [{self.B}, >= {rows}] with unit column stride on {meas.device}")
        n = C.c_int32()
        if _lib.lib().swd_frontend_push_dev(self._h, nbits, meas.data_ptr() if nbits else None, meas.stride(0) if nbits else 0, _is_packed(packed),
                                            out.data_ptr() if rows else None, out.stride(0) if rows else 0, C.byref(n), st.cuda_stream):
            raise _lib.error("swd_frontend_push_dev")
        return out[:, :rows] if out.shape[1] != rows else out

    def finish_device(self, final_meas, packed=False, stream=None):
        """``finish`` with a CUDA tensor, queued on ``stream`` -> (det_rows [B, rows] uint8, raw_obs [B] int32 bit masks), CUDA tensors"""
        import torch
        nbits = self._check_device_bits(final_meas, packed)
        rows = self.rows_for(nbits, final=True)
        st = torch.cuda.current_stream(final_meas.device) if stream is None else stream
        with torch.cuda.stream(st):
            out = torch.empty((self.B, rows), dtype=torch.uint8, device=final_meas.device)
            raw = torch.empty(self.B, dtype=torch.int32, device=final_meas.device)
        n = C.c_int32()
        if _lib.lib().swd_frontend_finish_dev(self._h, nbits, final_meas.data_ptr(), final_meas.stride(0), _is_packed(packed), out.data_ptr(),
                                              out.stride(0), C.byref(n), raw.data_ptr(), st.cuda_stream):
            raise _lib.error("swd_frontend_finish_dev")
        return out, raw


def _is_packed(packed):
    return 0 if packed is False or packed is None else 1


def _chunk_bits(width, packed):
    """bits of a chunk that is ``width`` bytes wide: ``packed`` False -> one per byte; True -> 8 per byte; an int -> that many bits
    of ceil(bits / 8) bytes (a packed chunk that ends inside a byte)"""
    if packed is False or packed is None:
        return int(width)
    if packed is True:
        return 8 * int(width)
    nbits = int(packed)
    if nbits < 0 or (nbits + 7) // 8 != width:
        raise ValueError(f"a packed chunk of {nbits} bits is {(nbits + 7) // 8} bytes wide, got {width}")
    return nbits


class _MeasurementSessionBase:
    """A ``MeasurementFrontEnd`` in front of a session: ``push`` takes measurement bits instead of detector rows and returns what
    the session's ``push`` returns for the rounds the bits completed."""

    def __init__(self, dec, session, mmap, max_shots, rows_per_round, num_obs):
        self.dec, self.session, self.frontend, self.B = dec, session, None, 0
        try:
            if mmap.n_half is not None and mmap.n_half != rows_per_round:
                raise ValueError(f"the map has {mmap.n_half} detector rows per round, the plan {rows_per_round}")
            if mmap.obs.shape[0] != num_obs:
                raise ValueError(f"the map has {mmap.obs.shape[0]} observables, the plan {num_obs}")
            self.frontend = MeasurementFrontEnd(mmap, rows_per_round, max_shots, dec.device)
        except Exception:
            session.close()
            raise

    def close(self):
        for x in (self.frontend, self.session):
            if x is not None:
                x.close()

    def begin(self, B):
        self.session.begin(B)
        self.frontend.begin(B)
        self.B = int(B)

    @property
    def bits_received(self):
        return self.frontend.bits_received

    def _check_push(self, nbits):
        pass  # (a rolling experiment has no length until it ends)

    def push(self, meas, packed=False):
        """meas [B, k] (host): the next bits of the syndrome rounds, any number; ``packed``: False = one byte per bit, True = 8 bits
        per byte, an int = that many bits in ceil(bits / 8) bytes.  Returns what the session's ``push`` returns for the detector rows
        of the rounds these bits completed."""
        fe = self.frontend
        d, nbits = fe._host_bits(meas, packed)
        self._check_push(nbits)
        return self.session.push(fe.push(d, packed))

    def push_device(self, meas, packed=False, stream=None, **kw):
        """The same with a uint8 CUDA tensor: the front end's launch, then the session's merge, decode and commit, are queued on
        ``stream`` (default: the current torch stream).  Returns what the session's ``push_device`` returns."""
        import torch
        fe = self.frontend
        nbits = fe._check_device_bits(meas, packed)
        self._check_push(nbits)
        st = torch.cuda.current_stream(meas.device) if stream is None else stream
        # the rows are a tensor of this push, allocated on its stream: a buffer kept from push to push would need an order of its
        # own when the stream changes (the front end's event is recorded before the session's merge has read the rows)
        return self.session.push_device(fe.push_device(meas, packed, stream=st), stream=st, **kw)


class MeasurementSession(_MeasurementSessionBase):
    """``SlidingWindowDecoder.measurement_session``: an online session (``SlidingWindowSession``) fed with the raw measurement record.
    ``push`` takes the bits of the syndrome rounds in pieces of any size; ``finish`` takes the rest of the last syndrome round and
    the final block, pushes the remaining detector rows -- the windows they complete are left in ``last_events``, in the form
    ``push`` returns them -- and returns the session's ``finish`` with the corrected readout."""

    def __init__(self, dec, max_shots, mmap):
        dec._no_loop("measurement_session()")
        if mmap.det.shape[0] != dec.num_det:
            raise ValueError(f"the map has {mmap.det.shape[0]} detectors, the plan {dec.num_det}")
        super().__init__(dec, dec.session(max_shots), mmap, max_shots, dec.plan.n_half, dec.num_obs)
        self.total_bits = self.frontend.blocks.rounds * self.frontend.meas_per_round
        self.last_events = []

    def _check_push(self, nbits):
        got = self.frontend.bits_received if self.B else 0
        if self.B and got + nbits > self.total_bits:
            raise ValueError(f"{nbits} bits after {got} received: the syndrome rounds of this experiment have {self.total_bits} "
                             f"(the final block of {self.frontend.meas_final} goes to finish)")

    def _check_finish(self, nbits):
        fe = self.frontend
        got = fe.bits_received if self.B else 0
        if self.B and got + nbits != self.total_bits + fe.meas_final:
            raise ValueError(f"finish: {nbits} bits after {got} received; the experiment has {self.total_bits} bits of syndrome rounds and a "
                             f"final block of {fe.meas_final}: finish takes the {self.total_bits + fe.meas_final - got} that are left")

    def finish(self, final_meas, packed=False):
        """final_meas [B, k] (host): the rest of the last syndrome round, if any, then the final block.  Returns ``(total_e_hat,
        stats, min_pm, obs_flips, flagged, raw_obs, logical_values)``: the first five as ``SlidingWindowSession.finish`` and
        ``decode`` leave them, ``raw_obs`` uint32 [B] = the observables' parities of the data measurement as read, and
        ``logical_values = raw_obs ^ obs_flips``, the corrected logical readout.  ValueError, with the state unchanged, unless the
        bits are exactly those the experiment still lacks."""
        fe = self.frontend
        d, nbits = fe._host_bits(final_meas, packed)
        self._check_finish(nbits)
        rows, raw = fe.finish(d, packed)
        self.last_events = self.session.push(rows)
        out = self.session.finish()
        return out + (raw, raw ^ out[3])


class RollingMeasurementSession(_MeasurementSessionBase):
    """``SlidingWindowDecoder.rolling_measurement_session``: a rolling session (``RollingSession``) fed with the raw measurement
    record of an experiment of any length the template serves; the map is that of the template's own R0 rounds.  The final block
    goes to ``finish``, with the rest of the last syndrome round if any: the rows of that round are pushed first -- the windows
    they complete are left in ``last_events``, in the form ``push`` returns them -- and the final block closes the experiment."""

    def __init__(self, dec, max_shots, mmap):
        dec._no_loop("rolling_measurement_session()")
        ses = dec.rolling_session(max_shots)
        super().__init__(dec, ses, mmap, max_shots, ses.template.n_half, dec.num_obs)
        self.last_events = []

    def finish(self, final_meas, packed=False):
        """final_meas [B, k] (host): the rest of the last syndrome round, if any, then the final block.  Returns ``(t, tail_faults,
        stats, min_pm, obs_flips, flagged, raw_obs, logical_values)``: the first six as ``RollingSession.finish`` returns them, then
        the raw observable parities and ``logical_values = raw_obs ^ obs_flips``.  ValueError, with the state unchanged, if the bits
        do not end the round under way and bring the final block, or the rounds are not a length the template serves."""
        fe, T = self.frontend, self.session.template
        d, nbits = fe._host_bits(final_meas, packed)
        ahead = fe.rows_for(nbits, final=True) - T.n_half  # rows of syndrome rounds the call completes
        rounds, rem = divmod(self.session.rows_received + ahead, T.n_half)
        if self.B and (rem or not T.serves(rounds)):
            raise ValueError(f"finish: the experiment would end after {rounds} syndrome rounds; this template serves {T.lengths()}")
        rows, raw = fe.finish(d, packed)
        self.last_events = self.session.push(rows[:, :ahead]) if ahead else []
        out = self.session.finish(rows[:, ahead:])
        return out + (raw, raw ^ out[4])


class DemSampler(_Handle):
    """Samples shots of a detector error model on the device: ``det, obs = sampler.sample(shots)`` is what
    ``dem.compile_sampler().sample(shots)`` gives the reference harness (/root/reference/osd.py:124-125).
    Faults are Bernoulli(priors) per column from a Philox4x32-10 stream that is a pure function of
    (seed, shot number, column): batches and ranks can be cut anywhere (``first_shot``)."""
    _destroy = "swd_sampler_destroy"

    def __init__(self, chk, obs, priors, device=0):
        L = _lib.lib()
        self._chk = _Csr(chk, priors)
        self.num_det, self.num_col = self._chk.m, self._chk.n
        self.num_obs = 0
        od = None
        if obs is not None:
            a = sp.csr_matrix(obs)
            a.sort_indices()
            self._orp, self._oci = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
            if a.shape[1] != self.num_col:
                raise ValueError(f"obs has {a.shape[1]} columns, chk has {self.num_col}")
            if a.shape[0] > 32:
                raise ValueError("at most 32 observables")
            self.num_obs = int(a.shape[0])
            od = _lib.GraphDesc(a.shape[0], a.shape[1], int(self._orp[-1]), self._orp.ctypes.data, self._oci.ctypes.data, None)
        self.device = int(device)
        self._h = L.swd_sampler_create(C.byref(self._chk.desc), C.byref(od) if od is not None else None, self.device)
        if not self._h:
            raise _lib.error("swd_sampler_create")

    def sample(self, shots, seed=20240318, first_shot=0, return_faults=False):
        """-> det uint8 [shots, num_det], obs uint8 [shots, num_obs] (, faults uint8 [shots, num_col])."""
        det = np.zeros((shots, self.num_det), np.uint8)
        flips = np.zeros(shots, np.uint32)
        faults = np.zeros((shots, self.num_col), np.uint8) if return_faults else None
        if _lib.lib().swd_sampler_sample(self._h, shots, int(seed), int(first_shot), det.ctypes.data, flips.ctypes.data,
                                         faults.ctypes.data if return_faults else None):
            raise _lib.error("swd_sampler_sample")
        obs = ((flips[:, None] >> np.arange(self.num_obs, dtype=np.uint32)) & 1).astype(np.uint8)
        return (det, obs, faults) if return_faults else (det, obs)

    def sample_device(self, shots, seed=20240318, first_shot=0, out=None, stream=None, faults=None):
        """-> torch tensors on the device: det uint8 [shots, num_det], observable-flip bit masks int32 [shots]; asynchronous on the
        current (or given) torch stream.  ``out`` = (det, flips) tensors to fill (contiguous, at least ``shots`` rows; ``flips`` None:
        the masks are not computed and None is returned for them); ``faults``: uint8 [>= shots, num_col], contiguous, receives the
        sampled faults."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = (torch.empty((shots, self.num_det), dtype=torch.uint8, device=dev), torch.empty((shots,), dtype=torch.int32, device=dev))
        det, flips = out
        st = torch.cuda.current_stream(dev) if stream is None else stream
        if _lib.lib().swd_sampler_sample_dev(self._h, shots, int(seed), int(first_shot), det.data_ptr(), 0,
                                             flips.data_ptr() if flips is not None else None,
                                             faults.data_ptr() if faults is not None else None, 0, st.cuda_stream):
            raise _lib.error("swd_sampler_sample_dev")
        return det[:shots], flips[:shots] if flips is not None else None


class CircuitSampler(_Handle):
    """Runs a memory circuit's op list (``circuit.bb_memory_ops``, ``shyps.shyps_memory_ops``) forwards on the device: a Pauli-frame
    simulation (``frames.py`` states the rule, C ABI swd_circuit_sampler_*).  ``measure`` / ``measure_device`` give the raw
    measurement record of every shot -- what ``MeasurementFrontEnd`` and the measurement sessions take; ``sample`` /
    ``sample_device`` give detectors and true observable flips in ``DemSampler``'s form, drawn from the circuit itself.  Every
    result is a pure function of (ops, seed, shot number).  ``randomize=False``: the record is the flips against the all-zero
    noiseless record; detectors and observables do not depend on it.  ``mmap``: the circuit's ``MeasurementMap``
    (``measurement_map(ops, n_half)``; ``n_half``, optional: the detector rows per round, which an op list does not mark and a
    measurement session asks its map for -- ``code.N // 2`` for the BB circuits; the sampler itself does not use it)."""
    _destroy = "swd_circuit_sampler_destroy"
    close = _Handle._release

    def __init__(self, ops, device=0, randomize=True, n_half=None):
        from .frames import compile_ops
        from .measurements import measurement_map
        self.program = prog = compile_ops(ops)  # ValueError names what is wrong with the list
        self.mmap = measurement_map(ops, n_half)
        self.device, self.randomize = int(device), bool(randomize)
        self.num_qubits, self.num_meas = prog.num_qubits, prog.num_meas
        self.num_det, self.num_obs = int(self.mmap.det.shape[0]), int(self.mmap.obs.shape[0])
        keep = []
        dd, od = _template_desc(self.mmap.det, keep), _template_desc(self.mmap.obs, keep)
        arrays = [np.ascontiguousarray(a) for a in (prog.kind, prog.qa, prog.qb, prog.thr, prog.meas, prog.noise_slot, prog.rand_slot)]
        self._h = _lib.lib().swd_circuit_sampler_create(len(prog), *[a.ctypes.data for a in arrays], prog.num_qubits, prog.num_meas,
                                                        C.byref(dd), C.byref(od), int(self.randomize), self.device)
        if not self._h:
            raise _lib.error("swd_circuit_sampler_create")

    def info(self):
        """dict: qubits, measurements, detectors, observables, noise_slots, random_slots, device_bytes, max_qubits"""
        v = (C.c_int64 * 8)()
        if _lib.lib().swd_circuit_sampler_info(self._h, v):
            raise _lib.error("swd_circuit_sampler_info")
        return dict(zip(("qubits", "measurements", "detectors", "observables", "noise_slots", "random_slots", "device_bytes", "max_qubits"), v))

    def record_bytes(self, packed=False):
        return (self.num_meas + 7) // 8 if packed else self.num_meas

    def measure(self, shots, seed=20240318, first_shot=0, packed=False):
        """-> the record uint8 [shots, num_meas] (host); ``packed``: [shots, ceil(num_meas / 8)], measurement i in bit ``i & 7`` of
        byte ``i >> 3`` (``np.packbits(..., bitorder="little")``, the front end's packed layout)"""
        meas = np.zeros((shots, self.record_bytes(packed)), np.uint8)
        if _lib.lib().swd_circuit_sampler_measure(self._h, shots, int(seed), int(first_shot), meas.ctypes.data, int(bool(packed))):
            raise _lib.error("swd_circuit_sampler_measure")
        return meas

    def sample(self, shots, seed=20240318, first_shot=0, return_measurements=False):
        """-> det uint8 [shots, num_det], obs uint8 [shots, num_obs] (, the record uint8 [shots, num_meas]) on the host"""
        det = np.zeros((shots, self.num_det), np.uint8)
        flips = np.zeros(shots, np.uint32)
        meas = np.zeros((shots, self.num_meas), np.uint8) if return_measurements else None
        if self.num_obs > 32:
            raise _lib.CapacityError(f"sample: observable masks carry at most 32 observables, the circuit has {self.num_obs}")
        if _lib.lib().swd_circuit_sampler_sample(self._h, shots, int(seed), int(first_shot), det.ctypes.data, flips.ctypes.data,
                                                 meas.ctypes.data if return_measurements else None):
            raise _lib.error("swd_circuit_sampler_sample")
        obs = ((flips[:, None] >> np.arange(self.num_obs, dtype=np.uint32)) & 1).astype(np.uint8)
        return (det, obs, meas) if return_measurements else (det, obs)

    def _check_out(self, t, shots, width, dtype, name):
        """a caller's tensor: on this sampler's device, ``dtype``, at least ``shots`` rows, [.., >= width] with unit column stride"""
        import torch
        want = torch.device("cuda", self.device)
        if not isinstance(t, torch.Tensor) or t.device != want:
            raise ValueError(f"{name} lives on {getattr(t, 'device', type(t).__name__)}, the sampler on {want}")
        ok = t.dtype == dtype and t.shape[0] >= shots
        if width is None:
            ok = ok and t.dim() == 1 and (t.shape[0] <= 1 or t.stride(0) == 1)
        else:
            ok = ok and t.dim() == 2 and t.shape[1] >= width and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= width)
        if not ok:
            raise ValueError(f"{name} must be a {dtype} tensor [>= {shots}" + (f", >= {width}] with unit column stride" if width is not None else "], contiguous"))

    def measure_device(self, shots, seed=20240318, first_shot=0, packed=False, out=None, stream=None):
        """-> the record as a uint8 CUDA tensor [shots, ``record_bytes(packed)``]; asynchronous on the current (or given) torch stream.
        ``out``: a uint8 CUDA tensor [>= shots, >= record bytes] with unit column stride to fill; bytes past a shot's record (a padded
        buffer) are left as they are."""
        import torch
        dev, row = torch.device("cuda", self.device), self.record_bytes(packed)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        if out is None:
            with torch.cuda.stream(st):
                out = torch.empty((shots, row), dtype=torch.uint8, device=dev)
        else:
            self._check_out(out, shots, row, torch.uint8, "out")
        if shots and _lib.lib().swd_circuit_sampler_measure_dev(self._h, shots, int(seed), int(first_shot), out.data_ptr(),
                                                                out.stride(0) if out.shape[0] > 1 else 0, int(bool(packed)), st.cuda_stream):
            raise _lib.error("swd_circuit_sampler_measure_dev")
        return out[:shots, :row]

    def sample_device(self, shots, seed=20240318, first_shot=0, out=None, stream=None, meas=None):
        """``DemSampler.sample_device``'s call: -> det uint8 [shots, num_det], observable-flip bit masks int32 [shots], CUDA tensors;
        asynchronous on the current (or given) torch stream.  ``out`` = (det, flips) tensors to fill (``flips`` None: no masks);
        ``meas``: uint8 [>= shots, >= num_meas], receives the record of the same shots."""
        import torch
        dev = torch.device("cuda", self.device)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        if out is None:
            with torch.cuda.stream(st):
                out = (torch.empty((shots, self.num_det), dtype=torch.uint8, device=dev), torch.empty((shots,), dtype=torch.int32, device=dev))
        det, flips = out
        self._check_out(det, shots, self.num_det, torch.uint8, "det")
        if flips is not None:
            self._check_out(flips, shots, None, torch.int32, "flips")
        if meas is not None:
            self._check_out(meas, shots, self.num_meas, torch.uint8, "meas")
        if shots and _lib.lib().swd_circuit_sampler_sample_dev(self._h, shots, int(seed), int(first_shot), det.data_ptr(),
                                                               det.stride(0) if det.shape[0] > 1 else 0,
                                                               flips.data_ptr() if flips is not None else None,
                                                               meas.data_ptr() if meas is not None else None,
                                                               meas.stride(0) if meas is not None and meas.shape[0] > 1 else 0, st.cuda_stream):
            raise _lib.error("swd_circuit_sampler_sample_dev")
        return det[:shots, :self.num_det], flips[:shots] if flips is not None else None


class PauliSampler(_Handle):
    """Samples Pauli errors of a CSS code and their syndromes on the device: what the first lines of the reference's data-noise
    cells compute with ``np.random.uniform`` and two dense products (/root/reference/Misc.ipynb cell 2:
    ``err_x = noise < px+py``, ``err_z = px < noise < px+py+pz``, ``syndrome_x = err_z @ hx.T``, ``syndrome_z = err_x @ hz.T``).
    The stream is Philox4x32-10, a pure function of (seed, shot number, qubit) (include/swd.h; tests/pauli_ref.py restates it):
    batches, lanes and ranks can be cut anywhere with ``first_shot``."""
    _destroy = "swd_pauli_sampler_destroy"

    def __init__(self, Hx, Hz, channel_probs_x, channel_probs_y, channel_probs_z, device=0):
        L = _lib.lib()
        if Hx.shape[1] != Hz.shape[1]:
            raise ValueError("Hx, Hz blocklength does not match!")
        n = Hx.shape[1]
        probs = [np.ascontiguousarray(v, dtype=np.float64) for v in (channel_probs_x, channel_probs_y, channel_probs_z)]
        for v in probs:
            if v.ndim != 1 or len(v) != n:
                raise ValueError(f"The length of the channel probability vector must be eqaul to the block length n={n}.")
        px, py, pz = probs
        if not all(((v >= 0.0) & (v <= 1.0)).all() for v in probs) or not ((px + py) + pz <= 1.0).all():
            raise ValueError("channel probabilities must lie in [0, 1] and px + py + pz must not exceed 1")
        self._px, self._py, self._pz = probs
        self._cx, self._cz = _Csr(Hx, px), _Csr(Hz, pz)
        self.mx, self.mz, self.n = self._cx.m, self._cz.m, n
        self.device = int(device)
        self._h = L.swd_pauli_sampler_create(C.byref(self._cx.desc), C.byref(self._cz.desc), px.ctypes.data, py.ctypes.data,
                                             pz.ctypes.data, self.device)
        if not self._h:
            raise _lib.error("swd_pauli_sampler_create")

    def sample(self, shots, seed=20240318, first_shot=0):
        """-> err uint8 [shots, 2, n] (row 0 the X string, row 1 the Z string), sx uint8 [shots, mx] = Hx err_z,
        sz uint8 [shots, mz] = Hz err_x."""
        err = np.zeros((shots, 2, self.n), np.uint8)
        sx, sz = np.zeros((shots, self.mx), np.uint8), np.zeros((shots, self.mz), np.uint8)
        if _lib.lib().swd_pauli_sampler_sample(self._h, shots, int(seed), int(first_shot), err.ctypes.data, sx.ctypes.data,
                                               sz.ctypes.data):
            raise _lib.error("swd_pauli_sampler_sample")
        return err, sx, sz

    def sample_device(self, shots, seed=20240318, first_shot=0, out=None, stream=None):
        """The same as torch uint8 tensors on the device, asynchronous on the current (or given) torch stream; ``out`` = (err, sx,
        sz) tensors to fill (contiguous, at least ``shots`` rows)."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = (torch.empty((shots, 2, self.n), dtype=torch.uint8, device=dev),
                   torch.empty((shots, self.mx), dtype=torch.uint8, device=dev),
                   torch.empty((shots, self.mz), dtype=torch.uint8, device=dev))
        err, sx, sz = out
        st = torch.cuda.current_stream(dev) if stream is None else stream
        if _lib.lib().swd_pauli_sampler_sample_dev(self._h, shots, int(seed), int(first_shot), err.data_ptr(), 0, sx.data_ptr(), 0,
                                                   sz.data_ptr(), 0, st.cuda_stream):
            raise _lib.error("swd_pauli_sampler_sample_dev")
        return err[:shots], sx[:shots], sz[:shots]


class _CssAccount(_Handle):
    """swd_css_account handle: ``cx`` = [Hx; Lx] on the Z string, ``cz`` = [Hz; Lz] on the X string, either None."""
    _destroy = "swd_css_account_destroy"

    def __init__(self, cx, stab_x, cz, stab_z, device):
        self._keep, descs = [], []
        for mat in (cx, cz):
            if mat is None:
                descs.append(None)
                continue
            a = sp.csr_matrix(mat)
            a.data = (np.asarray(a.data) % 2 != 0).astype(np.uint8)
            a.eliminate_zeros()
            a.sort_indices()
            rp, ci = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
            self._keep += [rp, ci]
            descs.append(_lib.GraphDesc(a.shape[0], a.shape[1], int(rp[-1]), rp.ctypes.data, ci.ctypes.data, None))
        self._h = _lib.lib().swd_css_account_create(C.byref(descs[0]) if descs[0] is not None else None, int(stab_x),
                                                    C.byref(descs[1]) if descs[1] is not None else None, int(stab_z), int(device))
        if not self._h:
            raise _lib.error("swd_css_account_create")

    def account(self, B, est, err, stats, result, counters, stream):
        """torch tensors (rows may be strided); ``stats`` / ``result`` / ``counters`` may be None."""
        if _lib.lib().swd_css_account_dev(self._h, B, est.data_ptr(), est.stride(0), err.data_ptr(), err.stride(0),
                                          stats.data_ptr() if stats is not None else None, STATUS_CONVERGE,
                                          result.data_ptr() if result is not None else None,
                                          counters.data_ptr() if counters is not None else None, stream.cuda_stream):
            raise _lib.error("swd_css_account_dev")


class _ErrorRate:
    """``ler`` and its standard error from a result's ``logical_errors`` and ``shots``."""

    @property
    def ler(self):
        return self.logical_errors / self.shots if self.shots else float("nan")

    @property
    def ler_stderr(self):
        """binomial standard error of ``ler``"""
        p = self.ler
        return float(np.sqrt(p * (1.0 - p) / self.shots)) if self.shots else float("nan")


class CodeCapacityResult(_ErrorRate):
    """Counters of a code-capacity run.  ``logical_errors``: shots whose correction leaves a logical error by the reference's
    criterion (a residual syndrome counts: it is not in ker(h) either); ``residual_syndromes``: those among them whose correction
    does not even reproduce the syndrome; ``not_converged``: shots with ``converge`` = 0 (the notebooks' "flagged");
    ``osd0_logical_errors``: logical errors of the OSD-0 solutions, None unless asked for."""

    def __init__(self, shots, logical_errors, residual_syndromes, not_converged, osd0_logical_errors=None):
        self.shots, self.logical_errors, self.residual_syndromes = int(shots), int(logical_errors), int(residual_syndromes)
        self.not_converged = int(not_converged)
        self.osd0_logical_errors = None if osd0_logical_errors is None else int(osd0_logical_errors)

    def _fields(self):
        return (self.shots, self.logical_errors, self.residual_syndromes, self.not_converged, self.osd0_logical_errors)

    def __eq__(self, other):
        return isinstance(other, CodeCapacityResult) and self._fields() == other._fields()

    def __repr__(self):
        return ("CodeCapacityResult(shots={}, logical_errors={}, residual_syndromes={}, not_converged={}, "
                "osd0_logical_errors={})".format(*self._fields()))


def _run_batches(shots, batch, lanes, first_shot, max_errors, enqueue, sync_lanes, logical_errors):
    """Which shots an experiment's ``run`` sends where, and when it may stop: batch j is ``min(batch, shots left)`` shots numbered
    from ``first_shot`` on, on lane ``j % lanes``.  With ``max_errors`` the count is read after every WHOLE round of lanes, once
    those lanes have been joined (a final partial round is not checked), and the loop stops at ``>= max_errors``.  The experiment
    supplies ``enqueue(lane, B, first shot of the batch)``, ``sync_lanes(lanes)`` and ``logical_errors()`` (the device counter);
    nothing here touches torch or the library.  -> shots enqueued."""
    start, k = 0, 0
    while start < shots:
        B = min(batch, shots - start)
        enqueue(k % lanes, B, first_shot + start)
        start, k = start + B, k + 1
        if max_errors is not None and k % lanes == 0:
            sync_lanes(lanes)
            if logical_errors() >= max_errors:
                break
    return start


class _LaneExperiment:
    """What the experiments share: the lanes -- a torch stream and buffers of its own each, ``dict(cap=, stream=, ...)`` -- and the
    frame of ``run``.  An experiment supplies ``_alloc(ln, cap, want)``, what a lane of ``cap`` shots holds (``want``: the buffer
    only some runs ask for), and ``_stale(ln, want)``, whether a lane that is large enough has to be set up again all the same."""

    def _stale(self, ln, want):
        return False

    def _lane(self, k, cap, want=False):
        import torch
        while len(self._lanes) <= k:  # (streams of both priorities: streams of one priority may share a hardware queue and then run back to back)
            self._lanes.append(dict(cap=0, stream=torch.cuda.Stream(torch.device("cuda", self.device), priority=-(len(self._lanes) & 1))))
        ln = self._lanes[k]
        if ln["cap"] < cap or self._stale(ln, want):
            ln["stream"].synchronize()  # (the buffers it replaces may still be in use)
            cap = max(cap, ln["cap"])
            ln.update(self._alloc(ln, cap, want), cap=cap)
        return ln

    def _sync_lanes(self, lanes=None):
        for ln in self._lanes[:lanes]:
            ln["stream"].synchronize()

    def _run(self, shots, batch, lanes, first_shot, max_errors, enqueue, logical_errors):
        """the caller has zeroed its device counters on the current stream; they are final when this returns"""
        import torch
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()  # the lanes add into zeroed counters
        _run_batches(shots, batch, lanes, first_shot, max_errors, enqueue, self._sync_lanes, logical_errors)
        self._sync_lanes()


class CodeCapacityExperiment(_LaneExperiment):
    """The reference's data-noise (code-capacity) Monte Carlo on the device: sample, decode, account, count -- only counters come
    back to the host.

    ``decoder="bp4_osd"`` with ``method="decode"`` is /root/reference/Misc.ipynb cell 2, with ``method="camel_decode"`` cell 8:
    Pauli errors from ``channel_probs_x / _y / _z`` (``PauliSampler``), ``bp4_osd(Hx, Hz, **decoder_kwargs)``, and the criterion
    ``(dz @ hz_perp.T).any() or (dx @ hx_perp.T).any()`` on the difference of estimate and error.  Cell 8's own codes -- the
    cycle-assembled and EG codes whose last qubit touches every check -- pass as ``(Hx, Hz)`` with ``osd_order=-1``
    (``bp4_osd``: up to 8 heavy columns; ``general_form=True`` among the decoder's keyword arguments takes any graph, such as
    the EG codes [[273,111,17]] and [[1057,571,33]]; ``general_osd=True`` runs ``decode`` with OSD on them); the sampler and the
    accounting have no degree bound.
    ``decoder`` in ``osd_window``, ``bpgdg_decoder``, ``bpgd_decoder``, ``bp_history_decoder`` is the single-basis harness of
    /root/reference/src/simulation.py: errors Bernoulli(``channel_probs``) (``DemSampler`` with ``chk = Hx``), syndrome
    ``err @ hx.T``, ``decoder(Hx, **decoder_kwargs)``, criterion ``(d @ hz_perp.T).any()``.

    ``code_or_matrices``: a ``codes.CSSCode`` or ``(Hx, Hz)``; ``lx`` / ``lz`` (keyword arguments, optional) are logical operators
    spanning ker(Hz) / rowspace(Hx) and ker(Hx) / rowspace(Hz), computed as ``codes.CSSCode`` does when absent."""

    _BINARY = {"osd_window": osd_window, "bpgdg_decoder": bpgdg_decoder, "bpgd_decoder": bpgd_decoder,
               "bp_history_decoder": bp_history_decoder}

    def __init__(self, code_or_matrices, decoder="bp4_osd", method="decode", device=0, **decoder_kwargs):
        from . import codes
        if decoder != "bp4_osd" and decoder not in self._BINARY:
            raise ValueError(f"unknown decoder '{decoder}': choose bp4_osd, " + ", ".join(self._BINARY))
        if method not in ("decode", "camel_decode") or (method == "camel_decode" and decoder != "bp4_osd"):
            raise ValueError(f"unknown method '{method}' for {decoder}: 'decode', or 'camel_decode' with bp4_osd")
        lx, lz = decoder_kwargs.pop("lx", None), decoder_kwargs.pop("lz", None)
        if isinstance(code_or_matrices, codes.CSSCode):
            code = code_or_matrices
        else:
            hx, hz = (m.toarray() if sp.issparse(m) else np.asarray(m) for m in code_or_matrices)
            code = codes.CSSCode(hx, hz, lx=lx, lz=lz)
        self.code, self.decoder_name, self.method, self.device = code, decoder, method, int(device)
        self.n, self.mx, self.mz = code.N, code.hx.shape[0], code.hz.shape[0]
        kw = dict(decoder_kwargs, device=self.device)
        if decoder == "bp4_osd":
            self.decoder = bp4_osd(code.hx, code.hz, **kw)
            self.sampler = PauliSampler(code.hx, code.hz, kw["channel_probs_x"], kw["channel_probs_y"], kw["channel_probs_z"],
                                        device=self.device)
            self._acct = _CssAccount(np.vstack([code.hx, code.lx]), self.mx, np.vstack([code.hz, code.lz]), self.mz, self.device)
        else:
            self.decoder = self._BINARY[decoder](code.hx, **kw)
            self.sampler = DemSampler(code.hx, None, kw["channel_probs"], device=self.device)
            self._acct = _CssAccount(np.vstack([code.hx, code.lx]), self.mx, None, 0, self.device)
        self._lanes = []

    # ---- one batch on one lane: sample, decode, account, all enqueued on the lane's stream -----------------------------------
    def _stale(self, ln, osd0):
        return osd0 and ln.get("osd0") is None

    def _alloc(self, ln, cap, osd0):
        import torch
        dev, u8 = torch.device("cuda", self.device), torch.uint8
        width = (2, self.n) if self.decoder_name == "bp4_osd" else (self.n,)
        return dict(err=torch.empty((cap,) + width, dtype=u8, device=dev), est=torch.empty((cap,) + width, dtype=u8, device=dev),
                    sx=torch.empty((cap, self.mx), dtype=u8, device=dev), sz=torch.empty((cap, self.mz), dtype=u8, device=dev),
                    stats=torch.empty((cap, _lib.STAT_WORDS), dtype=torch.int32, device=dev),
                    result=torch.empty((cap,), dtype=torch.int32, device=dev), result0=torch.empty((cap,), dtype=torch.int32, device=dev),
                    min_pm=torch.empty((cap,), dtype=torch.float64, device=dev),
                    osd0=torch.empty((cap,) + width, dtype=u8, device=dev) if osd0 else None)

    def _enqueue(self, ln, B, seed, first_shot, osd0, counters, counters0):
        import torch
        L, st, d = _lib.lib(), ln["stream"], self.decoder
        s = st.cuda_stream
        with torch.cuda.stream(st):
            if self.decoder_name == "bp4_osd":
                self.sampler.sample_device(B, seed, first_shot, out=(ln["err"], ln["sx"], ln["sz"]), stream=st)
                if self.method == "camel_decode":
                    rc = L.swd_bp4_camel_decode_batch_dev(d._h, B, ln["sx"].data_ptr(), ln["sz"].data_ptr(), ln["est"].data_ptr(),
                                                          ln["stats"].data_ptr(), None, s)
                else:
                    if osd0:  # (the decoder writes a shot's OSD-0 vector when BP converged or the OSD ran)
                        ln["osd0"][:B].zero_()
                    rc = L.swd_bp4_decode_batch_dev(d._h, B, ln["sx"].data_ptr(), ln["sz"].data_ptr(), ln["est"].data_ptr(),
                                                    ln["stats"].data_ptr(), None, ln["osd0"].data_ptr() if osd0 else None, None, s)
            else:
                self.sampler.sample_device(B, seed, first_shot, out=(ln["sx"], None), stream=st, faults=ln["err"])
                if self.decoder_name == "osd_window":
                    rc = L.swd_osdw_decode_batch_dev(d._h, B, ln["sx"].data_ptr(), 0, ln["est"].data_ptr(), 0, ln["stats"].data_ptr(),
                                                     ln["min_pm"].data_ptr(), None, 0, None, None, s)
                else:
                    rc = L.swd_gdg_decode_batch_dev(d._h, B, ln["sx"].data_ptr(), 0, ln["est"].data_ptr(), 0, ln["stats"].data_ptr(),
                                                    ln["min_pm"].data_ptr(), s)
            if rc:
                raise _lib.error(f"{self.decoder_name} device decode")
            self._acct.account(B, ln["est"], ln["err"], ln["stats"], ln["result"], counters, st)
            if osd0:
                self._acct.account(B, ln["osd0"], ln["err"], None, ln["result0"], counters0, st)

    def _check_osd0(self, osd0):
        if osd0 and not (self.decoder_name == "bp4_osd" and self.method == "decode"):
            raise ValueError("osd0=True needs decoder='bp4_osd' with method='decode'")

    def run(self, shots, batch=65536, seed=20240318, first_shot=0, lanes=4, osd0=False, max_errors=None):
        """``shots`` shots numbered ``first_shot ..`` in batches of ``batch`` that go round ``lanes`` streams (``bp4_osd`` has four
        launch slots), each lane with buffers of its own.  The host reads the counters once at the end; the result is then a pure
        function of (seed, first_shot, shots), whatever ``batch`` and ``lanes``.  With ``max_errors`` the counters are read after
        every round of lanes and the run stops once ``logical_errors >= max_errors``: it stops at batch granularity -- whole rounds of
        ``lanes`` batches -- so ``result.shots`` tells how many shots were run and the count may overshoot ``max_errors``.
        ``osd0=True`` (``bp4_osd`` / ``decode``) accounts the OSD-0 solutions in a second pass.  -> ``CodeCapacityResult``."""
        import torch
        shots, batch, lanes = int(shots), int(batch), int(lanes)
        if shots < 0 or batch <= 0 or lanes <= 0:
            raise ValueError("shots >= 0, batch > 0, lanes > 0")
        self._check_osd0(osd0)
        counters = torch.zeros((2, 4), dtype=torch.int64, device=torch.device("cuda", self.device))
        self._run(shots, batch, lanes, first_shot, max_errors,
                  lambda k, B, s: self._enqueue(self._lane(k, min(batch, shots), osd0), B, seed, s, osd0, counters[0], counters[1] if osd0 else None),
                  lambda: int(counters[0, 1].item()))
        c = counters.cpu().numpy()
        return CodeCapacityResult(c[0, 0], c[0, 1], c[0, 2], c[0, 3], c[1, 1] if osd0 else None)

    def run_batch(self, B, seed=20240318, first_shot=0, osd0=False):
        """One batch with the per-shot arrays on the host (tests and debugging): dict with ``err``, ``sx``, ``sz`` (``bp4_osd``:
        [B, 2, n] and both syndromes; binary decoders: [B, n], ``sx`` only), ``est``, ``stats`` [B, 8], ``result`` (the result words
        of include/swd.h: bit 0 logical error, bit 1 residual syndrome, bit 2 not converged) and, with ``osd0``, ``osd0`` /
        ``result_osd0``."""
        self._check_osd0(osd0)
        B = int(B)
        ln = self._lane(0, B, osd0)
        self._enqueue(ln, B, seed, int(first_shot), osd0, None, None)
        ln["stream"].synchronize()
        keys = ["err", "sx", "est", "stats", "result"] + (["sz"] if self.decoder_name == "bp4_osd" else [])
        out = {key: ln[key][:B].cpu().numpy() for key in keys}
        if osd0:
            out["osd0"], out["result_osd0"] = ln["osd0"][:B].cpu().numpy(), ln["result0"][:B].cpu().numpy()
        return out


def shot_account_device(shot_result, true_flips, stats=None, first_shot=0, result=None, counters=None, window_counters=None,
                        failed=None, stream=None):
    """swd_shot_account_dev on torch CUDA tensors (include/swd.h): ``shot_result`` int32 [B, 2] and ``true_flips`` int32 [B] as the
    window loop and the DEM sampler write them, ``stats`` int32 [B, W, 8] or None; ``result`` int32 [B], ``counters`` int64 [4],
    ``window_counters`` int64 [W, 10] and ``failed`` int64 [1 + cap] are optional outputs, the last three ADDED to (the caller zeroes
    them).  Asynchronous on the current (or given) torch stream."""
    import torch
    B, dev = int(shot_result.shape[0]), shot_result.device
    for name, t in (("shot_result", shot_result), ("true_flips", true_flips), ("stats", stats), ("result", result), ("counters", counters),
                    ("window_counters", window_counters), ("failed", failed)):
        if t is not None and (not t.is_cuda or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous CUDA tensor on {dev}")
    if tuple(shot_result.shape) != (B, 2) or shot_result.dtype != torch.int32 or tuple(true_flips.shape) != (B,) or true_flips.dtype != torch.int32:
        raise ValueError("shot_result must be int32 [B, 2] and true_flips int32 [B]")
    W = 0
    if stats is not None:
        if stats.dim() != 3 or stats.shape[0] != B or stats.shape[2] != _lib.STAT_WORDS or stats.dtype != torch.int32:
            raise ValueError(f"stats must be int32 [B, W, {_lib.STAT_WORDS}]")
        W = int(stats.shape[1])
    if result is not None and (result.dtype != torch.int32 or result.numel() < B):
        raise ValueError("result must be int32 [B]")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != 4):
        raise ValueError("counters must be int64 [4]")
    if window_counters is not None and (stats is None or window_counters.dtype != torch.int64
                                        or tuple(window_counters.shape) != (W, _lib.WINDOW_COUNTER_WORDS)):
        raise ValueError(f"window_counters needs stats and must be int64 [W, {_lib.WINDOW_COUNTER_WORDS}]")
    if failed is not None and (failed.dtype != torch.int64 or failed.dim() != 1 or failed.numel() < 1):
        raise ValueError("failed must be int64 [1 + cap]")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    if _lib.lib().swd_shot_account_dev(dev.index, B, W, ptr(shot_result), ptr(true_flips), ptr(stats), int(first_shot), ptr(result),
                                       ptr(counters), ptr(window_counters), ptr(failed), failed.numel() - 1 if failed is not None else 0,
                                       st.cuda_stream or None):
        raise _lib.error("swd_shot_account_dev")


def _observable_groups(groups, num_obs):
    """``observable_groups`` of the experiments' ``run`` -> (names, masks uint32 [G]) or None when there are none.  A group is a mask
    (an int) or a list of observable indices.  ValueError: more groups than one launch counts, an observable the plan does not have."""
    if not groups:
        return None
    if len(groups) > _lib.MAX_OBSERVABLE_GROUPS:
        raise ValueError(f"at most {_lib.MAX_OBSERVABLE_GROUPS} observable groups, got {len(groups)}")
    names, masks = [], []
    for name, g in dict(groups).items():
        if isinstance(g, (int, np.integer)):
            mask = int(g)
        else:
            idx = [int(i) for i in g]
            if any(i < 0 for i in idx):
                raise ValueError(f"observable group {name!r}: negative observable index")
            mask = 0
            for i in idx:
                mask |= 1 << i
        if mask < 0 or mask >> int(num_obs):
            raise ValueError(f"observable group {name!r} names an observable at or above the plan's {num_obs}")
        names.append(name)
        masks.append(mask)
    return names, np.array(masks, dtype=np.uint32)


def group_account_device(shot_result, true_flips, masks, counters, stream=None):
    """swd_group_account_dev on torch CUDA tensors (include/swd.h): ``shot_result`` int32 [B, 2] and ``true_flips`` int32 [B] as for
    ``shot_account_device``; ``masks``: up to 4 observable masks of 32 bits (host integers); ``counters`` int64 [len(masks)] is ADDED to
    with the shots whose predicted and true flips differ inside each mask (the caller zeroes it).  Asynchronous on the current (or
    given) torch stream."""
    import torch
    B, dev = int(shot_result.shape[0]), shot_result.device
    for name, t in (("shot_result", shot_result), ("true_flips", true_flips), ("counters", counters)):
        if not t.is_cuda or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous CUDA tensor on {dev}")
    if tuple(shot_result.shape) != (B, 2) or shot_result.dtype != torch.int32 or tuple(true_flips.shape) != (B,) or true_flips.dtype != torch.int32:
        raise ValueError("shot_result must be int32 [B, 2] and true_flips int32 [B]")
    m = [int(x) for x in masks]
    if len(m) > _lib.MAX_OBSERVABLE_GROUPS or any(x < 0 or x >> 32 for x in m):
        raise ValueError(f"at most {_lib.MAX_OBSERVABLE_GROUPS} masks of 32 bits")
    if counters.dtype != torch.int64 or counters.numel() != len(m):
        raise ValueError("counters must be int64 [len(masks)]")
    m = np.array(m, dtype=np.uint32)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    if _lib.lib().swd_group_account_dev(dev.index, B, shot_result.data_ptr(), true_flips.data_ptr(), len(m), m.ctypes.data, counters.data_ptr(),
                                        st.cuda_stream or None):
        raise _lib.error("swd_group_account_dev")


class MemoryResult(_ErrorRate):
    """Counters of a memory experiment under sliding windows -- what the reference's ``sliding_window_decoder`` prints
    (/root/reference/osd.py:181-194).  ``logical_errors``: shots that are flagged or whose predicted observable flips differ from
    the true ones ("Logical Errors"); ``flagged``: shots whose residual syndrome is not zero ("Overall Flagged Errors");
    ``observable_mismatches``: shots with a wrong observable, flagged or not.  Per window, or None when the run kept no window
    statistics: ``window_exit_classes`` [W, 8] (how many shots left window t through exit class c), ``window_not_converged`` [W]
    ("Window i, flagged Errors") and ``window_bp_iterations`` [W] (summed over the shots).  ``failed_shots``: sorted global numbers
    of shots with a logical error, at most ``keep_failures`` of the run; ``failed_shots_complete``: every such shot is in it (which
    shots an incomplete list holds is not reproducible, and ``==`` then leaves the list out).  ``group_errors``: name -> shots with a
    wrong observable inside that group of observables, for the ``observable_groups`` the run was asked for ({} when none)."""

    def __init__(self, shots, logical_errors, flagged, observable_mismatches, window_exit_classes=None, window_not_converged=None,
                 window_bp_iterations=None, failed_shots=None, failed_shots_complete=None, group_errors=None):
        self.shots, self.logical_errors, self.flagged = int(shots), int(logical_errors), int(flagged)
        self.observable_mismatches = int(observable_mismatches)
        as64 = lambda a: None if a is None else np.array(a, dtype=np.int64)  # noqa: E731
        self.window_exit_classes, self.window_not_converged = as64(window_exit_classes), as64(window_not_converged)
        self.window_bp_iterations = as64(window_bp_iterations)
        self.failed_shots = np.sort(np.array([] if failed_shots is None else failed_shots, dtype=np.uint64))
        self.failed_shots_complete = (len(self.failed_shots) == self.logical_errors) if failed_shots_complete is None \
            else bool(failed_shots_complete)
        self.group_errors = {k: int(v) for k, v in (group_errors or {}).items()}

    def ler_per_round(self, num_repeat):
        """osd.py:190-191: ``1 - (1 - ler) ** (1 / num_repeat)``"""
        return 1.0 - (1.0 - self.ler) ** (1.0 / num_repeat)

    def _fields(self):
        return (self.shots, self.logical_errors, self.flagged, self.observable_mismatches, self.failed_shots_complete)

    def __eq__(self, other):
        if not isinstance(other, MemoryResult) or self._fields() != other._fields() or self.group_errors != other.group_errors:
            return False
        for a, b in ((self.window_exit_classes, other.window_exit_classes), (self.window_not_converged, other.window_not_converged),
                     (self.window_bp_iterations, other.window_bp_iterations)):
            if (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
                return False
        return not self.failed_shots_complete or np.array_equal(self.failed_shots, other.failed_shots)

    __hash__ = None

    def __add__(self, other):
        """counters of two runs over disjoint shots (batches of a run, ranks that shard with ``first_shot``)"""
        if not isinstance(other, MemoryResult):
            return NotImplemented
        if set(self.group_errors) != set(other.group_errors):
            raise ValueError(f"results with observable groups {sorted(self.group_errors)} and {sorted(other.group_errors)} do not add")
        win = [None if a is None or b is None else a + b for a, b in
               ((self.window_exit_classes, other.window_exit_classes), (self.window_not_converged, other.window_not_converged),
                (self.window_bp_iterations, other.window_bp_iterations))]
        return MemoryResult(self.shots + other.shots, self.logical_errors + other.logical_errors, self.flagged + other.flagged,
                            self.observable_mismatches + other.observable_mismatches, *win,
                            failed_shots=np.concatenate([self.failed_shots, other.failed_shots]),
                            failed_shots_complete=self.failed_shots_complete and other.failed_shots_complete,
                            group_errors={k: v + other.group_errors[k] for k, v in self.group_errors.items()})

    def __repr__(self):
        s = "MemoryResult(shots={}, logical_errors={}, flagged={}, observable_mismatches={}".format(*self._fields()[:4])
        if self.group_errors:
            s += f", group_errors={self.group_errors}"
        if self.window_not_converged is not None:
            s += f", window_not_converged={self.window_not_converged.tolist()}"
        return s + f", failed_shots={len(self.failed_shots)}{'' if self.failed_shots_complete else ' (incomplete)'})"


class _MemoryLaneExperiment(_LaneExperiment):
    """What ``MemoryExperiment`` and ``RollingMemoryExperiment`` share beyond the lanes: the window decoder of a plan with 1..32
    observables, the device counters of a run and the result they make, and the frame of ``run_batch``."""

    observable_groups = None  # what ``run`` counts per group when it is not told (``phenomenological(basis="both")`` sets it)
    _device_loop = False      # whether the experiment runs on ``SlidingWindowDecoder(window_loop="device")``

    def __init__(self, plan, decoder, device, decoder_kwargs):
        num_obs = int(plan.obs.shape[0]) if plan.obs is not None else 0
        if num_obs == 0:
            raise ValueError("a memory experiment needs observables: plan.obs is empty")
        if num_obs > 32:
            raise ValueError(f"a memory experiment carries at most 32 observables per shot, plan.obs has {num_obs}")
        self.plan, self.device = plan, int(device)
        if decoder_kwargs.get("window_loop") == "device" and not self._device_loop:  # (before the window decoders are built)
            raise RuntimeError(f"{type(self).__name__} needs the one-launch pipeline: window_loop=\"device\" serves decode(), "
                               f"decode_device() and MemoryExperiment")
        self.decoder = SlidingWindowDecoder(plan, device=self.device, decoder=decoder, **decoder_kwargs)
        self.decoder._no_loop(type(self).__name__, device_ok=self._device_loop)
        self._lanes = []

    def _groups(self, observable_groups):
        """-> (names, (masks, zeroed device counters)) of ``observable_groups`` (None: the experiment's own), or (None, None)"""
        import torch
        g = _observable_groups(self.observable_groups if observable_groups is None else observable_groups, self.plan.obs.shape[0])
        if g is None:
            return None, None
        return g[0], (g[1], torch.zeros((len(g[1]),), dtype=torch.int64, device=torch.device("cuda", self.device)))

    @staticmethod
    def _group_errors(gnames, groups):
        return dict(zip(gnames, groups[1].cpu().tolist())) if groups is not None else None

    def _counters(self, window_rows, keep):
        """zeroed device counters of a run: shots, rows of window counters (0: none), numbers of failing shots to keep (0: none)"""
        import torch
        dev = torch.device("cuda", self.device)
        return (torch.zeros((4,), dtype=torch.int64, device=dev),
                torch.zeros((window_rows, _lib.WINDOW_COUNTER_WORDS), dtype=torch.int64, device=dev) if window_rows else None,
                torch.zeros((1 + keep,), dtype=torch.int64, device=dev) if keep else None)

    def _result(self, counters, wc, failed, keep, gnames, groups):
        """after the lanes were joined: the pipeline's status is checked, the device counters are read once -> (args, kwargs) of
        ``MemoryResult``"""
        self.decoder.check_status()
        c = counters.cpu().numpy()
        w = wc.cpu().numpy() if wc is not None else None
        kept = failed.cpu().numpy().view(np.uint64) if failed is not None else np.zeros(1, np.uint64)
        return (c[0], c[1], c[2], c[3]) + ((w[:, :8], w[:, 8], w[:, 9]) if w is not None else (None, None, None)), \
            dict(failed_shots=kept[1:1 + min(int(kept[0]), keep)], failed_shots_complete=int(c[1]) <= keep,
                 group_errors=self._group_errors(gnames, groups))

    def _run_one_batch(self, B, observable_groups, enqueue, keys, want=False):
        """the frame of ``run_batch``: ``enqueue(ln, groups)`` on lane 0, then ``keys`` of the lane and the true flips on the host"""
        import torch
        gnames, groups = self._groups(observable_groups)
        if groups is not None:
            torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()  # the lane adds into zeroed counters
        ln = self._lane(0, B, want)
        enqueue(ln, groups)
        ln["stream"].synchronize()
        self.decoder.check_status()
        out = {key: ln[key][:B].cpu().numpy() for key in keys}
        out["true_flips"] = ln["flips"][:B].cpu().numpy().view(np.uint32)
        if groups is not None:
            out["group_errors"] = self._group_errors(gnames, groups)
        return out


class MemoryExperiment(_MemoryLaneExperiment):
    """The reference's ``sliding_window_decoder(N, p, num_repeat, num_shots, W, F, ...)`` (/root/reference/osd.py:123-194, guessing.py)
    on the device: sample the detector error model (``DemSampler``), run the (W, F) window loop (``SlidingWindowDecoder``), compare
    the predicted observable flips with the true ones and reduce the per-window records -- only counters come back to the host.

    ``plan``: a ``windows.WindowPlan`` with 1..32 observables that the one-launch pipeline takes; ``decoder`` and the keyword
    arguments are those of ``SlidingWindowDecoder``.  ``sampler``: None -- the ``DemSampler`` of the plan -- or an object with
    ``DemSampler.sample_device``'s call that draws ``plan.chk.shape[0]`` detectors in the plan's row order (``CircuitSampler``).  With ``window_loop="device"`` any plan the single-window decoders take,
    the ones beyond the pipeline kernels included: the lanes of ``run`` are then torch streams that call ``decode_device`` of
    the one window-loop handle, whose decodes are ordered on the device (general-form windows also join their previous
    stream on the host when the stream changes), so two lanes overlap sampling and accounting with the loop, not two loops."""

    _device_loop = True

    def __init__(self, plan, decoder="osd_window", device=0, sampler=None, **decoder_kwargs):
        if sampler is not None:  # (before the window decoders are built)
            if not callable(getattr(sampler, "sample_device", None)):
                raise ValueError("sampler must be None (the DemSampler of the plan) or an object with DemSampler's sample_device")
            if getattr(sampler, "num_det", None) != plan.chk.shape[0]:
                raise ValueError(f"the sampler draws {getattr(sampler, 'num_det', None)} detectors, the plan has {plan.chk.shape[0]}")
            if getattr(sampler, "device", int(device)) != int(device):
                raise ValueError(f"the sampler lives on device {sampler.device}, the experiment on device {int(device)}")
        super().__init__(plan, decoder, device, decoder_kwargs)
        self.sampler = DemSampler(plan.chk, plan.obs, plan.priors, device=self.device) if sampler is None else sampler
        self.W = self.decoder.W
        self._stream = None

    @classmethod
    def bb(cls, N, p, num_repeat, W, F, method=1, z_basis=True, decoder="osd_window", sampler=None, **kw):
        """the plan as the notebooks build it: ``bb_code(N)``, ``bb_dem(code, A, B, p, num_repeat, z_basis)``, ``plan_windows``.
        ``sampler="circuit"``: the shots are drawn from the circuit itself -- ``CircuitSampler(bb_memory_ops(...))``, whose
        detectors are in the plan's row order (the plan permutes columns only) -- instead of from the detector error model."""
        from .circuit import bb_dem, bb_memory_ops
        from .codes import bb_code
        from .windows import plan_windows
        code, A, B = bb_code(N)
        dem = bb_dem(code, A, B, p, num_repeat, z_basis=z_basis)
        if isinstance(sampler, str):
            if sampler != "circuit":
                raise ValueError(f"sampler: None, \"circuit\" or a sampler object, got {sampler!r}")
            sampler = CircuitSampler(bb_memory_ops(code, A, B, p, num_repeat, z_basis), device=kw.get("device", 0), n_half=N // 2)
        return cls(plan_windows(dem.chk, dem.obs, dem.priors, N // 2, W, F, method, z_basis), decoder=decoder, sampler=sampler, **kw)

    @classmethod
    def phenomenological(cls, code_or_matrices, p, num_repeat, W, F, q=None, basis="z", noise="bitflip", decoder="osd_window", **kw):
        """the memory experiment of ANY CSS code under phenomenological noise (``phenomenological.css_phenomenological_dem``): data
        faults with probability ``p`` before each of ``num_repeat`` rounds and before the final exact one, measurement faults with
        probability ``q`` (``None``: ``p``).  ``code_or_matrices``: a ``codes.CSSCode``, or a pair ``(H, logicals)`` where there is none.
        The plan is ``plan_windows(..., n_half=<detectors per round>, method=0)``: the generic windows (``method=1`` hard-codes the BB
        circuit's column offsets), which end in the identity block of the last round's measurement faults by themselves.
        ``basis="both"`` counts the Z and the X logical errors apart by default: ``observable_groups = {"z": the first k
        observables, "x": the last k}``."""
        from .phenomenological import experiment_model
        from .windows import plan_windows
        dem, n_half, groups = experiment_model(code_or_matrices, p, num_repeat, q, basis, noise)
        exp = cls(plan_windows(dem.chk, dem.obs, dem.priors, n_half, W, F, method=0), decoder=decoder, **kw)
        exp.observable_groups = groups
        return exp

    def close(self):
        if getattr(self, "_stream", None) is not None:
            self._stream.close()
            self._stream = None

    __del__ = close

    # ---- one batch on one lane: sample, window loop, account, all ordered on the lane's torch stream ---------------------------
    def _stale(self, ln, window_stats):
        return window_stats and ln.get("stats") is None

    def _alloc(self, ln, cap, window_stats):
        import torch
        dev, d, i32 = torch.device("cuda", self.device), self.decoder, torch.int32
        return dict(det=torch.empty((cap, d.num_det), dtype=torch.uint8, device=dev), flips=torch.empty((cap,), dtype=i32, device=dev),
                    total=torch.empty((cap, d.num_col), dtype=torch.uint8, device=dev), shot_result=torch.empty((cap, 2), dtype=i32, device=dev),
                    result=torch.empty((cap,), dtype=i32, device=dev),
                    stats=torch.empty((cap, self.W, _lib.STAT_WORDS), dtype=i32, device=dev) if window_stats or ln.get("stats") is not None else None)

    def _enqueue(self, ln, B, seed, first_shot, streamed, window_stats, counters, window_counters, failed, groups=None):
        """``groups``: (masks, counters int64 [len(masks)]) or None"""
        st, d = ln["stream"], self.decoder
        total, shot, stats = ln["total"][:B], ln["shot_result"][:B], ln["stats"][:B] if window_stats else None
        det = self.sampler.sample_device(B, seed, first_shot, out=(ln["det"], ln["flips"]), stream=st)[0]
        if streamed:  # the stream object's lane starts behind the sampler; the accounting waits for that lane alone
            self._stream.push_device(det, total, stats=stats, min_pm=None, shot_result=shot, after=st)
            self._stream.wait_last(st)
        else:
            d.decode_device(det, total=total, stats=stats, shot_result=shot, stream=st, want_stats=window_stats, want_min_pm=False)
        shot_account_device(shot, ln["flips"][:B], stats, first_shot, ln["result"], counters, window_counters, failed, stream=st)
        if groups is not None:
            group_account_device(shot, ln["flips"][:B], groups[0], groups[1], stream=st)

    def run(self, shots, batch=4096, seed=20240318, first_shot=0, lanes=2, max_errors=None, keep_failures=0, window_stats=True,
            observable_groups=None):
        """``shots`` shots numbered ``first_shot ..`` in batches of ``batch``.  ``lanes=2``: batch j goes to lane ``j & 1`` of one
        ``SlidingWindowStream``, each lane with a torch stream and buffers of its own, so that two batches are in flight;
        ``lanes=1``: ``decode_device`` launches on one stream.  The host reads the counters once at the end; the result is a pure
        function of (seed, first_shot, shots), whatever ``batch`` and ``lanes``.  With ``max_errors`` the counters are read after every
        round of lanes and the run stops once ``logical_errors >= max_errors``: it stops at batch granularity -- whole rounds of
        ``lanes`` batches -- so ``result.shots`` tells how many shots were run and the count may overshoot ``max_errors``.
        ``keep_failures``: how many numbers of failing shots to bring back; ``window_stats=False`` leaves the per-window records
        out (the window loop then writes none).  ``observable_groups``: name -> observable mask or list of observable indices, at
        most 4; ``result.group_errors[name]`` then counts the shots with a wrong observable inside the group, in one more small launch
        per batch (none without groups; ``{}`` switches the experiment's own groups off).  -> ``MemoryResult``."""
        shots, batch, lanes, keep = int(shots), int(batch), int(lanes), int(keep_failures)
        if shots < 0 or batch <= 0 or lanes not in (1, 2) or keep < 0:
            raise ValueError("shots >= 0, batch > 0, lanes 1 or 2 (a stream object has two), keep_failures >= 0")
        gnames, groups = self._groups(observable_groups)
        cap = max(1, min(batch, shots))
        streamed = lanes == 2 and self.decoder.window_loop == "pipeline"  # (the device window loop has no stream object: two torch streams)
        if streamed and (self._stream is None or self._stream.max_shots < cap):
            self._sync_lanes()
            self.close()
            self._stream = self.decoder.stream(cap, want_stats=window_stats)
        counters, wc, failed = self._counters(self.W if window_stats else 0, keep)
        self._run(shots, batch, lanes, first_shot, max_errors,
                  lambda k, B, s: self._enqueue(self._lane(k, cap, window_stats), B, seed, s, streamed, window_stats, counters, wc, failed, groups),
                  lambda: int(counters[1].item()))
        args, kw = self._result(counters, wc, failed, keep, gnames, groups)
        return MemoryResult(*args, **kw)

    def run_batch(self, B, seed=20240318, first_shot=0, observable_groups=None):
        """One batch with the per-shot arrays on the host (tests and debugging): dict with ``det`` [B, num_det], ``true_flips`` uint32
        [B], ``total`` [B, num_col], ``stats`` [B, W, 8], ``shot_result`` [B, 2] and ``result`` (the words of include/swd.h: bit 0
        logical error, bit 1 flagged, bit 2 observable mismatch); with ``observable_groups`` (as in ``run``) also ``group_errors``."""
        B = int(B)
        if B <= 0:
            raise ValueError("B > 0")
        return self._run_one_batch(B, observable_groups,
                                   lambda ln, groups: self._enqueue(ln, B, seed, int(first_shot), False, True, None, None, None, groups),
                                   ("det", "total", "stats", "shot_result", "result"), want=True)


class RollingDemSampler(_Handle):
    """Samples the detector rows of a memory experiment of ANY number of rounds from a template of R0 rounds, a few row blocks (of
    ``n_half`` rows) per call and bit-identical to ``DemSampler`` on the model of that many rounds (C ABI: swd_rolling_sampler_*;
    ``windows.extend_template`` with the Philox stream on the global column number is the executable specification).  Its device
    memory is the template's.  ``template_plan``: a ``windows.WindowPlan`` that ``windows.rolling_template`` accepts, or the
    ``RollingTemplate`` itself; ``from_blocks`` takes any periodic model."""
    _destroy = "swd_rolling_sampler_destroy"

    def __init__(self, template_plan, device=0):
        from .windows import _as_template, template_blocks
        T = _as_template(template_plan)  # ValueError names what is not periodic
        j0, j1, cols = template_blocks(T)
        self._create(T.plan.chk, T.plan.obs, T.plan.priors, T.n_half, j0, j1, cols, device)
        self.template, self.min_rounds = T, max(self.min_rounds, int(T.min_rounds))

    @classmethod
    def from_blocks(cls, chk, obs, priors, n_half, j0, j1, anchor_cols, device=0):
        """a periodic model given as ``windows.extend_periodic`` takes it: column blocks ``j0 .. j1 - 1`` are the body rounds"""
        self = cls.__new__(cls)
        self.template = None
        self._create(chk, obs, priors, n_half, j0, j1, anchor_cols, device)
        return self

    def _create(self, chk, obs, priors, n_half, j0, j1, anchor_cols, device):
        L = _lib.lib()
        self._h = None
        self._chk = _Csr(chk, priors)
        self.num_col = self._chk.n
        od = None
        if obs is not None and obs.shape[0]:
            a = sp.csr_matrix(obs)
            a.sort_indices()
            if a.shape[0] > 32:
                raise ValueError(f"at most 32 observables, obs has {a.shape[0]}")
            self._orp, self._oci = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
            od = _lib.GraphDesc(a.shape[0], a.shape[1], int(self._orp[-1]), self._orp.ctypes.data, self._oci.ctypes.data, None)
        cols = np.ascontiguousarray(anchor_cols, dtype=np.int64)
        self.device = int(device)
        self._h = L.swd_rolling_sampler_create(C.byref(self._chk.desc), C.byref(od) if od is not None else None, int(n_half), int(j0), int(j1),
                                               cols.ctypes.data, len(cols) - 1, self.device)
        if not self._h:
            raise _lib.error("swd_rolling_sampler_create", prefix_value=True)
        info = (C.c_int32 * 8)()
        L.swd_rolling_sampler_info(self._h, info, -1, 0, 0, None, None)
        self.n_half, self.num_obs, self.R0, self.min_rounds = int(info[0]), int(info[2]), int(info[3]), int(info[6])

    def _check_rounds(self, rounds):
        if int(rounds) < self.min_rounds:
            serves = f"this template serves {self.template.lengths()}" if self.template is not None else f"at least {self.min_rounds}"
            raise ValueError(f"{rounds} rounds are fewer than the template's shortest experiment: {serves}")

    def columns(self, rounds, block0=0, nblocks=None):
        """(first column, number of columns) of column blocks ``block0 .. block0 + nblocks - 1`` (default: to the end) of the model of
        ``rounds`` rounds"""
        self._check_rounds(rounds)
        nblocks = int(rounds) + 1 - int(block0) if nblocks is None else int(nblocks)
        c0, nc = C.c_int64(), C.c_int64()
        if _lib.lib().swd_rolling_sampler_info(self._h, None, int(rounds), int(block0), nblocks, C.byref(c0), C.byref(nc)):
            raise ValueError(f"swd_rolling_sampler_info failed: {_lib.last_error()}")
        return c0.value, nc.value

    def rows_device(self, shots, rounds, block0, nblocks, seed=20240318, first_shot=0, out=None, flips=None, stream=None, faults=None):
        """One stateless call on the device: rows ``[block0 * n_half, (block0 + nblocks) * n_half)`` of shots ``first_shot ..`` of the
        ``rounds``-round experiment into ``out`` (uint8 CUDA tensor [shots, nblocks * n_half] with unit column stride -- a column
        slice of a wider tensor fits; allocated when None).  ``flips`` int32 [shots] is XORed INTO with the observable masks of the
        faults in column blocks ``block0 .. block0 + nblocks - 1`` (None: not computed); ``faults`` uint8 [shots, columns of those
        blocks] likewise optional.  Asynchronous on ``stream`` (default: the current torch stream).  -> ``out``."""
        import torch
        dev = torch.device("cuda", self.device)
        shots, nrows = int(shots), int(nblocks) * self.n_half
        ncols = self.columns(rounds, block0, nblocks)[1]  # ValueError: rounds or blocks out of range
        if out is None:
            out = torch.empty((shots, nrows), dtype=torch.uint8, device=dev)
        for name, t, shape, dt in (("out", out, (shots, nrows), torch.uint8), ("flips", flips, (shots,), torch.int32),
                                   ("faults", faults, (shots, ncols), torch.uint8)):
            if t is not None and (not t.is_cuda or t.device != dev or t.dtype != dt or tuple(t.shape) != shape
                                  or (t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1) or (t.dim() == 1 and not t.is_contiguous())):
                raise ValueError(f"{name} must be a {dt} CUDA tensor {list(shape)} on {dev} with unit column stride")
        st = torch.cuda.current_stream(dev) if stream is None else stream
        if _lib.lib().swd_rolling_sampler_rows_dev(self._h, shots, int(seed), int(first_shot), int(rounds), int(block0), int(nblocks), out.data_ptr(),
                                                   out.stride(0) if shots > 1 else 0, flips.data_ptr() if flips is not None else None,
                                                   faults.data_ptr() if faults is not None else None,
                                                   faults.stride(0) if faults is not None and shots > 1 else 0, st.cuda_stream or None):
            raise _lib.error("swd_rolling_sampler_rows_dev")
        return out

    def sample(self, shots, rounds, seed=20240318, first_shot=0, return_faults=False):
        """The whole experiment of ``rounds`` rounds on the host (tests and debugging): det uint8 [shots, (rounds + 1) * n_half], obs
        uint8 [shots, num_obs] (, faults uint8 [shots, columns of the model]) -- what ``DemSampler`` on the model of ``rounds`` rounds
        returns for the same seed and shot numbers."""
        ncols = self.columns(rounds)[1]
        det = np.zeros((shots, (int(rounds) + 1) * self.n_half), np.uint8)
        flips = np.zeros(shots, np.uint32)
        faults = np.zeros((shots, ncols), np.uint8) if return_faults else None
        if _lib.lib().swd_rolling_sampler_rows(self._h, shots, int(seed), int(first_shot), int(rounds), 0, int(rounds) + 1, det.ctypes.data,
                                               flips.ctypes.data, faults.ctypes.data if return_faults else None):
            raise _lib.error("swd_rolling_sampler_rows")
        obs = ((flips[:, None] >> np.arange(self.num_obs, dtype=np.uint32)) & 1).astype(np.uint8)
        return (det, obs, faults) if return_faults else (det, obs)


class RollingMemoryResult(MemoryResult):
    """``MemoryResult`` of a rolling experiment of ``rounds`` syndrome rounds (``windows_per_shot`` windows a shot).  The per-window
    arrays have THREE rows whatever the length: the head window, all body windows summed, the tail window.  Results of different
    ``rounds`` do not add."""

    def __init__(self, rounds, windows_per_shot, *args, **kw):
        super().__init__(*args, **kw)
        self.rounds, self.windows_per_shot = int(rounds), int(windows_per_shot)

    def ler_per_round(self, num_repeat=None):
        return super().ler_per_round(self.rounds if num_repeat is None else num_repeat)

    def _fields(self):
        return super()._fields() + (self.rounds, self.windows_per_shot)

    def __eq__(self, other):
        return isinstance(other, RollingMemoryResult) and super().__eq__(other)

    __hash__ = None

    def __add__(self, other):
        if not isinstance(other, RollingMemoryResult):
            return NotImplemented
        if other.rounds != self.rounds:
            raise ValueError(f"results of experiments of {self.rounds} and of {other.rounds} rounds do not add")
        s = MemoryResult.__add__(self, other)
        return RollingMemoryResult(self.rounds, self.windows_per_shot, s.shots, s.logical_errors, s.flagged, s.observable_mismatches,
                                   s.window_exit_classes, s.window_not_converged, s.window_bp_iterations, failed_shots=s.failed_shots,
                                   failed_shots_complete=s.failed_shots_complete, group_errors=s.group_errors)

    def __repr__(self):
        return "Rolling" + super().__repr__()[:-1] + f", rounds={self.rounds})"


def _smallest_rolling_template(num_repeat, W, F, make_plan, short_form):
    """The plan of the least ``R0 = num_repeat (mod F)``, ``W <= R0 <= num_repeat``, that ``windows.rolling_template`` accepts.
    ``make_plan(R0)`` -> (plan of R0 rounds, whatever else the caller wants back with it); ``short_form``: the constructor to
    recommend when there is none.  -> what ``make_plan`` returned for that R0; ValueError relays the last refusal."""
    from . import windows
    num_repeat, why = int(num_repeat), "none was tried"
    R0 = W + (num_repeat - W) % F
    while R0 <= num_repeat:
        plan, extras = make_plan(R0)
        try:
            windows.rolling_template(plan)
        except ValueError as e:
            why, R0 = f"R0 = {R0}: {e}", R0 + F
            continue
        return plan, extras
    raise ValueError(f"no rolling template serves {num_repeat} rounds with (W, F) = ({W}, {F}): it needs R0 = {num_repeat} (mod {F}), "
                     f"R0 <= {num_repeat}, periodic between its first and its last window, and {why}.  Use {short_form} for "
                     f"an experiment this short")


class RollingMemoryExperiment(_MemoryLaneExperiment):
    """``MemoryExperiment`` for experiments of any length: the reference's ``sliding_window_decoder(N, p, num_repeat, ...)`` swept over
    ``num_repeat`` from ONE template plan of R0 rounds, in device memory that does not depend on the length.  Per batch and lane:
    ``RollingSession.begin``; per window the rows it still needs from ``RollingDemSampler`` and one window step of the session;
    the tail rows and ``finish``; the accounting of ``MemoryExperiment``.  Only counters come back.  The result equals
    ``MemoryExperiment(plan_windows(rounds)).run`` for the same seed and shot numbers, the per-window counts reduced to head / body
    / tail.  ``template_plan``: a ``windows.WindowPlan`` with 1..32 observables that the one-launch pipeline takes and
    ``windows.rolling_template`` accepts; it serves ``rounds = R0 (mod F)``, ``rounds >= min_rounds``."""

    def __init__(self, template_plan, decoder="osd_window", device=0, **decoder_kwargs):
        from .windows import rolling_template
        super().__init__(template_plan, decoder, device, decoder_kwargs)
        self.template = rolling_template(template_plan)  # ValueError names what is not periodic
        self.sampler = RollingDemSampler(self.template, device=self.device)
        T = self.template
        self.rounds = int(T.R0)  # the default length of run()
        # row blocks a step hands over at most: the head's W, a body window's F, what finish takes
        self._step_blocks = max(T.W, T.F, (T.tail.row1 - T.tail.row0) // T.n_half - (T.W - T.F))

    @classmethod
    def bb(cls, N, p, num_repeat, W, F, method=1, z_basis=True, decoder="osd_window", **kw):
        """the experiment of ``num_repeat`` rounds as the notebooks build it, on the SMALLEST template that serves it: the plan of
        ``bb_dem(bb_code(N), p, R0)`` with the least ``R0 = num_repeat (mod F)``, ``R0 <= num_repeat``, that ``rolling_template``
        accepts.  ``run()`` then defaults to ``num_repeat`` rounds."""
        from .circuit import bb_dem
        from .codes import bb_code
        from .windows import plan_windows
        code, A, B = bb_code(N)

        def make_plan(R0):
            dem = bb_dem(code, A, B, p, R0, z_basis=z_basis)
            return plan_windows(dem.chk, dem.obs, dem.priors, N // 2, W, F, method, z_basis), None
        exp = cls(_smallest_rolling_template(num_repeat, W, F, make_plan, "MemoryExperiment.bb")[0], decoder=decoder, **kw)
        exp.rounds = int(num_repeat)
        return exp

    @classmethod
    def phenomenological(cls, code_or_matrices, p, num_repeat, W, F, q=None, basis="z", noise="bitflip", decoder="osd_window", **kw):
        """``MemoryExperiment.phenomenological`` for experiments of any length, built as ``bb`` builds its own: on the SMALLEST
        template that serves ``num_repeat`` -- the model of the least ``R0 = num_repeat (mod F)``, ``R0 <= num_repeat``, that
        ``rolling_template`` accepts.  ``run()`` then defaults to ``num_repeat`` rounds."""
        from .phenomenological import experiment_model
        from .windows import plan_windows

        def make_plan(R0):
            dem, n_half, groups = experiment_model(code_or_matrices, p, R0, q, basis, noise)
            return plan_windows(dem.chk, dem.obs, dem.priors, n_half, W, F, method=0), groups
        plan, groups = _smallest_rolling_template(num_repeat, W, F, make_plan, "MemoryExperiment.phenomenological")
        exp = cls(plan, decoder=decoder, **kw)
        exp.rounds, exp.observable_groups = int(num_repeat), groups
        return exp

    def close(self):
        for ln in getattr(self, "_lanes", []):
            ln["stream"].synchronize()
            if ln.get("session") is not None:
                ln["session"].close()
        self._lanes = []

    __del__ = close

    @property
    def device_bytes(self):
        """bytes of device memory the lanes own (sessions and buffers): a function of the template, the batch and the lanes used --
        not of the number of rounds"""
        return sum(ln["session"].device_bytes + sum(t.numel() * t.element_size() for t in ln.values() if hasattr(t, "element_size"))
                   for ln in self._lanes)

    # ---- one batch on one lane: per window sample + step (+ its counts), then the tail and the accounting, all on the lane's stream ---
    def _alloc(self, ln, cap, want):
        import torch
        dev, i32 = torch.device("cuda", self.device), torch.int32
        if ln.get("session") is not None:  # a session serves the shots it was opened for: a larger lane opens another
            ln["session"].close()
        return dict(session=self.decoder.rolling_session(cap),
                    rows=torch.empty((cap, self._step_blocks * self.template.n_half), dtype=torch.uint8, device=dev),
                    flips=torch.empty((cap,), dtype=i32, device=dev), shot_result=torch.empty((cap, 2), dtype=i32, device=dev),
                    result=torch.empty((cap,), dtype=i32, device=dev), stats=torch.empty((cap, _lib.STAT_WORDS), dtype=i32, device=dev))

    def _enqueue(self, ln, B, rounds, sched, seed, first_shot, window_stats, counters, window_counters, failed, det=None, stats_all=None,
                 groups=None):
        """``det`` [B, (rounds + 1) * n_half] / ``stats_all`` [windows, B, 8]: run_batch's own arrays, written instead of the lane's;
        ``groups``: (masks, counters int64 [len(masks)]) or None"""
        import torch
        L, h, ses = _lib.lib(), self.template.n_half, ln["session"]
        sp_ = ln["stream"].cuda_stream
        flips, shot = ln["flips"], ln["shot_result"]
        first, count = C.c_int64(), C.c_int32()
        ses.begin(B)
        with torch.cuda.stream(ln["stream"]):
            flips[:B].zero_()
        for k, (b0, n) in enumerate(sched):
            last = k == len(sched) - 1
            rows = ln["rows"] if det is None else det[:, b0 * h:]
            stats = ln["stats"] if stats_all is None else stats_all[k]
            if L.swd_rolling_sampler_rows_dev(self.sampler._h, B, int(seed), int(first_shot), rounds, b0, n, rows.data_ptr(), rows.stride(0),
                                              flips.data_ptr(), None, 0, sp_):
                raise _lib.error("swd_rolling_sampler_rows_dev")
            sptr = stats.data_ptr() if window_stats else None
            if not last:
                if L.swd_pipeline_rolling_push_dev(ses._h, n * h, rows.data_ptr(), rows.stride(0), 1, None, sptr, None, C.byref(first),
                                                   C.byref(count), sp_) or count.value != 1 or first.value != k:
                    raise RuntimeError(f"swd_pipeline_rolling_push_dev failed at window {k}: {_lib.last_error()}")
                if window_stats and window_counters is not None:  # the counts of this window alone, into the row of its kind
                    if L.swd_shot_account_dev(self.device, B, 1, shot.data_ptr(), flips.data_ptr(), sptr, 0, None, None,
                                              window_counters[min(k, 1)].data_ptr(), None, 0, sp_):
                        raise _lib.error("swd_shot_account_dev")
                continue
            if L.swd_pipeline_rolling_finish_dev(ses._h, n * h, rows.data_ptr(), rows.stride(0), None, sptr, None, shot.data_ptr(), sp_):
                raise _lib.error("swd_pipeline_rolling_finish_dev")
            wins = window_stats and window_counters is not None
            if L.swd_shot_account_dev(self.device, B, 1 if wins else 0, shot.data_ptr(), flips.data_ptr(), sptr if wins else None, int(first_shot),
                                      ln["result"].data_ptr(), counters.data_ptr() if counters is not None else None,
                                      window_counters[2].data_ptr() if wins else None, failed.data_ptr() if failed is not None else None,
                                      failed.numel() - 1 if failed is not None else 0, sp_):
                raise _lib.error("swd_shot_account_dev")
            if groups is not None:
                group_account_device(shot[:B], flips[:B], groups[0], groups[1], stream=ln["stream"])

    def _schedule(self, rounds):
        from .windows import rolling_schedule
        rounds = self.rounds if rounds is None else int(rounds)
        return rounds, rolling_schedule(self.template, rounds)  # ValueError names the lengths served

    def run(self, shots, rounds=None, batch=4096, seed=20240318, first_shot=0, lanes=2, max_errors=None, keep_failures=0, window_stats=True,
            observable_groups=None):
        """``shots`` shots numbered ``first_shot ..`` of the experiment of ``rounds`` syndrome rounds (default: the template's, or what
        ``bb`` was asked for) in batches of ``batch``; batch j goes to lane ``j % lanes``, each lane a torch stream, a
        ``RollingSession`` and buffers of its own -- ``[batch, rows of one step]``, whatever ``rounds``.  The host reads the counters
        once at the end; the result is a pure function of (seed, first_shot, shots, rounds), whatever ``batch`` and ``lanes``.
        ``max_errors``, ``keep_failures``, ``window_stats`` and ``observable_groups`` as in ``MemoryExperiment.run``.  ValueError, before anything is
        launched, when the template does not serve ``rounds``.  -> ``RollingMemoryResult``."""
        shots, batch, lanes, keep = int(shots), int(batch), int(lanes), int(keep_failures)
        if shots < 0 or batch <= 0 or lanes not in (1, 2) or keep < 0:
            raise ValueError("shots >= 0, batch > 0, lanes 1 or 2, keep_failures >= 0")
        rounds, sched = self._schedule(rounds)
        cap = max(1, min(batch, shots))
        gnames, groups = self._groups(observable_groups)
        counters, wc, failed = self._counters(3 if window_stats else 0, keep)
        self._run(shots, batch, lanes, first_shot, max_errors,
                  lambda k, B, s: self._enqueue(self._lane(k, cap), B, rounds, sched, seed, s, window_stats, counters, wc, failed, groups=groups),
                  lambda: int(counters[1].item()))
        args, kw = self._result(counters, wc, failed, keep, gnames, groups)
        return RollingMemoryResult(rounds, len(sched), *args, **kw)

    def run_batch(self, B, rounds=None, seed=20240318, first_shot=0, observable_groups=None):
        """One batch with the per-shot arrays on the host (tests and debugging; unlike ``run`` it holds the whole experiment's rows):
        dict with ``det`` [B, (rounds + 1) * n_half], ``true_flips`` uint32 [B], ``stats`` [B, windows, 8], ``shot_result`` [B, 2] and
        ``result`` (the words of include/swd.h: bit 0 logical error, bit 1 flagged, bit 2 observable mismatch); with
        ``observable_groups`` (as in ``run``) also ``group_errors``."""
        import torch
        B = int(B)
        if B <= 0:
            raise ValueError("B > 0")
        rounds, sched = self._schedule(rounds)
        own = {}  # the whole experiment's rows and every window's records: this call's own arrays, not the lane's

        def enqueue(ln, groups):
            dev = torch.device("cuda", self.device)
            with torch.cuda.stream(ln["stream"]):
                own["det"] = torch.empty((B, (rounds + 1) * self.template.n_half), dtype=torch.uint8, device=dev)
                own["stats"] = torch.empty((len(sched), B, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
            self._enqueue(ln, B, rounds, sched, seed, int(first_shot), True, None, None, None, det=own["det"], stats_all=own["stats"],
                          groups=groups)
        out = self._run_one_batch(B, observable_groups, enqueue, ("shot_result", "result"))
        out.update(det=own["det"].cpu().numpy(), stats=np.ascontiguousarray(own["stats"].cpu().numpy().transpose(1, 0, 2)))
        return out
