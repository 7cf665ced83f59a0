"""Python front-end of the sum-check vector kernels (row N2 of SURVEY.md 8f).

Mirrors the host helpers of src/backend/r1cs_helper.rs as Reef's witness generator drives them
(src/backend/r1cs.rs:2318-2385): `gen_eq_table`, then per round `linear_mle_product` split into its
two halves around the Poseidon challenge, which stays on the host.  Values are canonical Python
ints (the reference uses rug::Integer); all arithmetic runs in libreef_msm.so.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

import numpy as np

from . import _ffi
from ._fe import _Handle, _arr, _ints
from ._ffi import REEF_DEVICE, REEF_HOST, check
from .msm import curve_id

ints_to_array = _arr        # the public names of _fe's pair: Python ints <-> (n, 4) uint64 arrays of little-endian limbs
array_to_ints = _ints


_SYMBOL_BYTES = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.uint32): 4}


def _symbol_bytes(dtype) -> int:
    """1, 2 or 4 for the unsigned symbol types; anything signed or wider is refused -- its values are never wrapped silently."""
    try:
        return _SYMBOL_BYTES[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError(f"document symbols are uint8, uint16 or uint32, not {dtype!r}") from None


def sc_part_descriptors(parts):
    """The parts of SumCheck.set_table_parts as reef_sc_part structures, and the host arrays their pointers point into (keep them
    until the call has returned).  No device is touched."""
    descs, keep = [], []
    for part in parts:
        kind = part[0]
        if kind == "fe" and len(part) == 2:
            arr = part[1] if isinstance(part[1], np.ndarray) else ints_to_array(part[1])
            arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
            keep.append(arr)
            descs.append(_ffi.ScPart(_ffi.SC_PART_FE, 0, arr.ctypes.data if arr.shape[0] else None, arr.shape[0], REEF_HOST))
        elif kind == "symbols" and len(part) == 2:
            if not isinstance(part[1], np.ndarray):
                raise ValueError("host symbols are a numpy array of uint8, uint16 or uint32")
            eb = _symbol_bytes(part[1].dtype)
            arr = np.ascontiguousarray(part[1]).reshape(-1)
            keep.append(arr)
            descs.append(_ffi.ScPart(_ffi.SC_PART_SYMBOLS, eb, arr.ctypes.data if arr.size else None, arr.size, REEF_HOST))
        elif kind == "symbols" and len(part) == 4:
            buf, dtype, count = part[1:]
            eb = _symbol_bytes(dtype)
            ptr = buf.ptr if hasattr(buf, "ptr") else int(buf)
            if hasattr(buf, "nbytes") and int(count) * eb > buf.nbytes:
                raise ValueError("device buffer too small")
            keep.append(buf)
            descs.append(_ffi.ScPart(_ffi.SC_PART_SYMBOLS, eb, ptr, int(count), REEF_DEVICE))
        elif kind == "fill" and len(part) == 3:
            arr = ints_to_array([part[1]])
            keep.append(arr)
            descs.append(_ffi.ScPart(_ffi.SC_PART_FILL, 0, arr.ctypes.data, int(part[2]), REEF_HOST))
        else:
            raise ValueError(f"not a part of a sum-check table: {part[0]!r} with {len(part) - 1} values")
    return descs, keep


class SumCheck(_Handle):
    """Resident (T, EQ) tables of 2^ell entries over the scalar field of `curve`."""
    _destroy = "reef_sc_destroy"

    def __init__(self, curve, ell: int):
        self._lib = _ffi.load()
        self.ell = ell
        self.len = 1 << ell
        h = ctypes.c_void_p()
        check(self._lib.reef_sc_create(ctypes.byref(h), curve_id(curve), self.len))
        self._h = h

    def set_table(self, which: int, values) -> None:
        """values: list of ints, or an (n, 4) uint64 array of canonical limbs."""
        arr = values if isinstance(values, np.ndarray) else ints_to_array(values)
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        self._pending = None
        check(self._lib.reef_sc_set_table(self._h, which, arr.ctypes.data, arr.shape[0], REEF_HOST))

    def set_table_device(self, which: int, ptr: int, n: int) -> None:
        self._pending = None
        check(self._lib.reef_sc_set_table(self._h, which, ptr, n, REEF_DEVICE))

    def set_table_parts(self, parts) -> None:
        """T <- the parts laid end to end from entry 0, zero beyond them (reef_sc_set_table_parts).  A part is one of
        ("fe", ints | (n, 4) uint64 array), ("symbols", uint8 / uint16 / uint32 ndarray), ("symbols", DeviceBuffer, dtype, count)
        and ("fill", value, count).  Reef's "nldoc" table is [("symbols", doc)], its "nlhybrid" table
        [("fe", table), ("fill", calc_fill, half - len(table)), ("symbols", proj_doc)]."""
        descs, keep = sc_part_descriptors(parts)
        arr = (_ffi.ScPart * max(1, len(descs)))(*descs)
        self._pending = None
        check(self._lib.reef_sc_set_table_parts(self._h, arr, len(descs)))
        del keep

    def gen_eq_table(self, rs: Sequence[int], qs: Sequence[int], last_q: Sequence[int]) -> None:
        """gen_eq_table(rs, qs, last_q) (r1cs_helper.rs:508-544) into the EQ table."""
        assert len(rs) == len(qs) + 1 and len(last_q) == self.ell
        a, lq = ints_to_array(rs), ints_to_array(last_q)
        q = np.ascontiguousarray(np.array(list(qs) + [0], dtype=np.uint32))
        self._pending = None
        check(self._lib.reef_sc_gen_eq_table(self._h, a.ctypes.data, q.ctypes.data, len(qs), lq.ctypes.data, self.ell))

    def round_coeffs(self, i: int) -> Tuple[int, int, int]:
        """First half of linear_mle_product for round i in 1..ell: (xsq, x, con)."""
        out = np.zeros((3, 4), dtype=np.uint64)
        check(self._lib.reef_sc_round_coeffs(self._h, 1 << (self.ell - i), out.ctypes.data))
        xsq, x, con = array_to_ints(out)
        return xsq, x, con

    def fold(self, i: int, r: int) -> None:
        """Second half of linear_mle_product for round i with the host's challenge r."""
        rr = ints_to_array([r])
        self._pending = None
        check(self._lib.reef_sc_fold(self._h, 1 << (self.ell - i), rr.ctypes.data))

    def fold_and_next_coeffs(self, i: int, r: int) -> Tuple[int, int, int]:
        """fold(i, r) fused with round_coeffs(i + 1): one pass over the tables (i < ell)."""
        rr = ints_to_array([r])
        out = np.zeros((3, 4), dtype=np.uint64)
        self._pending = None
        check(self._lib.reef_sc_fold_and_next_coeffs(self._h, 1 << (self.ell - i), rr.ctypes.data, out.ctypes.data))
        xsq, x, con = array_to_ints(out)
        return xsq, x, con

    def linear_mle_product(self, i: int, sponge) -> Tuple[int, int, int, int]:
        """The whole of the reference's linear_mle_product(table_t, table_eq, ell, i, sponge) (src/backend/r1cs_helper.rs:441-506) on the
        resident tables: the round's sums, absorb (con, x, xsq) in that order (:478-482), squeeze the challenge (:485-488), fold both
        tables.  Returns (r_i, xsq, x, con) like the reference.  `sponge` is the caller's transcript (absorb(list of ints), squeeze(n) ->
        list: the SpongeAPI calls Reef makes; neptune's on the Rust side): the challenge is the host's.  Rounds driven one after the
        other as r1cs.rs:2318-2385 does cost one pass over the tables each: the fold of round i also yields round i + 1's sums."""
        pending = getattr(self, "_pending", None)
        xsq, x, con = pending[1] if pending is not None and pending[0] == i else self.round_coeffs(i)
        sponge.absorb([con, x, xsq])
        r_i = sponge.squeeze(1)[0]
        if i < self.ell:
            self._pending = (i + 1, self.fold_and_next_coeffs(i, r_i))
        else:
            self.fold(i, r_i)
            self._pending = None
        return r_i, xsq, x, con

    def read(self, which: int, count: int) -> List[int]:
        out = np.zeros((count, 4), dtype=np.uint64)
        check(self._lib.reef_sc_read(self._h, which, count, out.ctypes.data))
        return array_to_ints(out)

    def lookup(self, idx: Sequence[int], out=None):
        """T[idx[j]] of the table as last set (what reset_table restores), however far T has been folded: the v_i of a step's lookups
        (r1cs.rs:2066-2077).  Does not disturb the rounds: a pending fused round stays pending.  Returns the list of ints, or -- out: a
        DeviceBuffer of 32 bytes per index -- writes them there as canonical integers and returns None."""
        q = np.ascontiguousarray(np.array([int(i) for i in idx], dtype=np.uint64))
        if out is not None:
            if out.nbytes < 32 * len(q):
                raise ValueError("device buffer too small")
            check(self._lib.reef_sc_lookup(self._h, q.ctypes.data, len(q), out.ptr, REEF_DEVICE))
            return None
        host = np.zeros((len(q), 4), dtype=np.uint64)
        check(self._lib.reef_sc_lookup(self._h, q.ctypes.data, len(q), host.ctypes.data, REEF_HOST))
        return array_to_ints(host)

    def reset_table(self) -> None:
        """T <- the table as last set (start of the next folding step)."""
        self._pending = None
        check(self._lib.reef_sc_reset_table(self._h))

    def sync(self) -> None:
        check(self._lib.reef_sc_sync(self._h))
