"""Record / replay of the calls tests/test_oracle_vs_ref.py makes into the reference's own C/C++ objects (oracle/_ref/libswd_ref.so).

Where the library exists the tests call it live; with SWD_RECORD_REF=1 every call is also written to
tests/golden/ref_calls/<test>.npz.  Where it does not exist (its sources are not part of this repository), the tests replay that
file: each call must arrive with the same function, scalar arguments and input buffers (compared by hash) as the recorded one, and
gets the reference's recorded return value and output buffers back.  So an oracle that feeds the reference different inputs, or
answers differently from it, fails in both modes."""
from __future__ import annotations

import ctypes as C
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls")


def _buf(addr, nbytes):
    return C.string_at(addr, nbytes) if nbytes else b""


def _cell(arg):
    """the c_double behind C.byref(x)"""
    return arg._obj


class RefCalls:
    """Stands in for the CDLL: attribute access gives a callable per exported function (argtypes / restype set on it are kept for
    the live library and ignored in replay)."""

    def __init__(self, test_id, lib=None, record=False):
        self.lib, self.record = lib, record
        self.path = os.path.join(GOLDEN, test_id.replace("[", "-").replace("]", "") + ".npz")
        self.dims = {}       # handle -> (m, n) of a parity-check matrix or a BPGD object, (m, new_n) of an ensemble object
        self.ids = {}        # live handle -> the number of the call that made it (hashed instead of the address)
        self.log = []        # (input hash, return value, output bytes)
        self.pos = self.ncalls = 0
        if lib is None:
            if not os.path.exists(self.path):
                raise FileNotFoundError(f"no recorded reference calls at {self.path} and no oracle/_ref/libswd_ref.so")
            f = np.load(self.path)
            self.hashes, self.rets, self.outs, self.out_ofs = f["hashes"], f["rets"], f["outs"], f["out_ofs"]

    def __getattr__(self, name):
        if not name.startswith("ref_"):
            raise AttributeError(name)
        fn = _Fn(self, name)
        object.__setattr__(self, name, fn)
        return fn

    def _hid(self, h):
        return self.ids[h] if self.lib is not None else h

    def call(self, name, fn, args):
        if name.endswith("_free"):  # (nothing to compare; a destructor may run after the test has finished)
            return fn(*args) if fn is not None else None
        ins, outs, new_dims = self._spec(name, args)
        scalars = tuple(float(x) if isinstance(x, (float, np.floating)) else int(x) for x in ins[0])
        key = hashlib.blake2b(repr((name, scalars)).encode() + b"".join(ins[1:]), digest_size=8).digest()
        key = np.frombuffer(key, np.uint64)[0]
        if self.lib is not None:
            ret = fn(*args)
            if self.record:
                data = b"".join(np.float64(_cell(o).value).tobytes() if n is None else _buf(o, n) for o, n in outs)
                self.log.append((key, 0 if ret is None else ret, data))
        else:
            i = self.pos
            assert i < len(self.hashes), f"{name}: more reference calls than recorded ({len(self.hashes)})"
            assert self.hashes[i] == key, f"{name}: call {i} differs in its inputs from the recorded reference call"
            self.pos += 1
            data = self.outs[self.out_ofs[i]:self.out_ofs[i + 1]].tobytes()
            k = 0
            for o, n in outs:
                if n is None:
                    _cell(o).value = float(np.frombuffer(data[k:k + 8], np.float64)[0])
                    k += 8
                else:
                    C.memmove(o, data[k:k + n], n)
                    k += n
            ret = self.rets[i]
            ret = float(ret) if name == "ref_bpgd_get_pm" else int(ret)
        self.ncalls += 1
        if name.endswith("_new"):  # handles are hashed as the number of the call that made them
            if self.lib is not None:
                self.ids[ret] = self.ncalls
            else:
                ret = self.ncalls
        if new_dims is not None:
            self.dims[ret] = new_dims
        return ret

    def _spec(self, name, a):
        """(inputs: [scalar tuple, buffers...], outputs: [(address or byref cell, bytes or None for a double)], dims of a new handle)"""
        d = self.dims
        if name == "ref_pcm_new":
            m, n, rp, ci = a
            nnz = int(np.frombuffer(_buf(rp + 4 * m, 4), np.int32)[0])
            return [(m, n), _buf(rp, 4 * (m + 1)), _buf(ci, 4 * nnz)], [], (m, n)
        if name in ("ref_rank", "ref_bpgd_min_sum_log", "ref_bpgd_get_pm"):
            return [(self._hid(a[0]),)], [], None
        if name == "ref_index_sort":
            v, cols, n = a
            return [(n,), _buf(v, 8 * n)], [(cols, 4 * n)], None
        if name == "ref_osd0":
            h, rank, cols, s, out = a
            m, n = d[h]
            return [(self._hid(h), rank), _buf(cols, 4 * n), _buf(s, m)], [(out, n)], None
        if name == "ref_bpgd_new":
            return [tuple(a)], [], (a[0], a[1])
        if name == "ref_bpgd_reset":
            b, h, cols, llr, s = a
            m, n = d[h]
            return [(self._hid(b), self._hid(h)), _buf(cols, 4 * n), _buf(llr, 8 * n), _buf(s, m)], [], None
        if name == "ref_bpgd_decimate_vn_reliable":
            return [(self._hid(a[0]), a[1], a[2])], [], None
        if name == "ref_bpgd_error":
            b, out = a
            return [(self._hid(b),)], [(out, d[b][1])], None
        if name == "ref_gdg_multi":
            h, m, new_n = a[0], a[1], a[2]
            cols, llr, s, err, pm, pms = a[11:]
            n = d[h][1]
            return ([(self._hid(h),) + tuple(a[1:11]), _buf(cols, 4 * n), _buf(llr, 8 * n), _buf(s, m)],
                    [(err, new_n), (pm, None), (pms, 8 * 256)], None)
        if name == "ref_gdg_multi_new":
            return [tuple(a)], [], (a[0], a[1])
        if name == "ref_gdg_multi_decode":
            o, h, m, new_n, cols, llr, s, err, pm, pms = a
            n = d[h][1]
            return ([(self._hid(o), self._hid(h), m, new_n), _buf(cols, 4 * n), _buf(llr, 8 * n), _buf(s, m)],
                    [(err, new_n), (pm, None), (pms, 8 * 256)], None)
        raise NotImplementedError(name)

    def finish(self):
        """recording: write the log; replay: every recorded call must have been made"""
        if self.lib is not None:
            if self.record:
                os.makedirs(GOLDEN, exist_ok=True)
                outs = [x[2] for x in self.log]
                np.savez_compressed(self.path, hashes=np.array([x[0] for x in self.log], np.uint64),
                                    rets=np.array([x[1] for x in self.log], np.float64),
                                    outs=np.frombuffer(b"".join(outs), np.uint8),
                                    out_ofs=np.cumsum([0] + [len(o) for o in outs]).astype(np.int64))
        else:
            assert self.pos == len(self.hashes), f"{len(self.hashes) - self.pos} recorded reference calls were not made"


class _Fn:
    def __init__(self, owner, name):
        self.owner, self.name = owner, name
        self.fn = getattr(owner.lib, name) if owner.lib is not None else None

    def __setattr__(self, k, v):
        if k in ("argtypes", "restype"):
            if self.fn is not None:
                setattr(self.fn, k, v)
            return
        object.__setattr__(self, k, v)

    def __call__(self, *args):
        return self.owner.call(self.name, self.fn, args)
