"""Python front-end of the Hyrax consistency argument on a resident document (include/reef_msm.h 3i).

NLDocCommitment::proof_dot_prod_prover -> HyraxPC::prove_eval (Reef: src/backend/commitment.rs:287-405): the bound rows LZ = L^T Z,
the evaluation <LZ, R>, the blind combination sum_i L_i blind_i, optionally comm_LZ = sum_i L_i C_i, then the IPA rounds of 3h over
gens_v with an optional blinding term on a second point h.  The document stays on the device from `HyraxEval(...)` on; only
challenges and blinds go in, only points and single scalars come out.  `prove_eval` drives a whole argument with a caller-supplied
`challenge(label, absorbed) -> int` in place of the transcript.  Scalars cross as Python ints (canonical, or pasta Montgomery form
with is_mont=True); points as numpy uint64 arrays in the C-ABI layouts: affine (8 limbs) in, Jacobian (12 limbs) out.
"""
from __future__ import annotations

import ctypes
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import REEF_DEVICE, REEF_HOST, check
from .msm import DeviceBuffer, MsmContext, curve_id
from ._fe import _Handle, _arr, _ints, _mont_forms
from .spartan import _ipa_rounds, compress

_ELEM = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 2, np.dtype(np.uint32): 4, np.dtype(np.int32): 4}


def _table(z, n: Optional[int] = None, elem_bytes: Optional[int] = None) -> Tuple[int, int, int, int]:
    """(loc, ptr, n, elem_bytes) of a document: symbols of 1 / 2 / 4 bytes (uint8, uint16 / int16, uint32 / int32: read as unsigned),
    or field elements as an (n, 4) array of 64-bit limbs (uint64 / int64), C-contiguous, in host memory; or a reef_amd.msm.DeviceBuffer
    on the ctx's device with n and elem_bytes given (it must hold n * elem_bytes bytes).  Anything else is refused."""
    if isinstance(z, DeviceBuffer):
        if n is None or elem_bytes not in (1, 2, 4, 32):
            raise ValueError("a device document needs n and elem_bytes (1, 2, 4 or 32)")
        if z.nbytes < n * elem_bytes:
            raise ValueError(f"the device buffer holds {z.nbytes} bytes, {n} entries of {elem_bytes} need {n * elem_bytes}")
        return REEF_DEVICE, z.ptr, n, elem_bytes
    if not isinstance(z, np.ndarray):
        raise TypeError("the document is a numpy array or a reef_amd.msm.DeviceBuffer")
    if not z.flags["C_CONTIGUOUS"]:
        raise ValueError("the document array must be C-contiguous")
    if z.dtype in _ELEM:
        return REEF_HOST, z.ctypes.data, z.size, _ELEM[z.dtype]
    if z.dtype in (np.dtype(np.uint64), np.dtype(np.int64)) and z.ndim == 2 and z.shape[1] == 4:
        return REEF_HOST, z.ctypes.data, z.shape[0], 32
    raise TypeError(f"a document array holds uint8/uint16/int16/uint32/int32 symbols or (n, 4) 64-bit limbs, not {z.dtype} {z.shape}")


def factored_lens(num_vars: int) -> Tuple[int, int]:
    """compute_factored_lens (commitment.rs:173-174): (left, right) = (num_vars / 2, num_vars - num_vars / 2)"""
    return num_vars // 2, num_vars - num_vars // 2


class HyraxEval(_Handle):
    """The committed matrix Z (2^left x 2^right, row-major, the document zero-padded to 2^num_vars) resident on one device, with
    its row blinds.  z: symbols of 1 / 2 / 4 bytes or an (n, 4) array of field elements (is_mont form), as a numpy array, or a
    DeviceBuffer with n and elem_bytes (device memory, copied); see _table for what is accepted."""
    _destroy = "reef_hyrax_destroy"

    def __init__(self, curve, z, num_vars: int, left_vars: Optional[int] = None, *, row_blinds: Optional[Sequence[int]] = None,
                 is_mont: bool = False, device: int = 0, n: Optional[int] = None, elem_bytes: Optional[int] = None):
        self._lib = _ffi.load()
        self.curve = curve_id(curve)
        self.num_vars = num_vars
        self.left = factored_lens(num_vars)[0] if left_vars is None else left_vars
        self.right = num_vars - self.left
        loc, ptr, n, eb = _table(z, n, elem_bytes)
        self._keep = z
        self.n, self.elem_bytes = n, eb
        rb = None
        if row_blinds is not None:
            rb = _arr(row_blinds)
            if rb.shape[0] != 1 << self.left:
                raise ValueError(f"expected {1 << self.left} row blinds, got {rb.shape[0]}")
        h = ctypes.c_void_p()
        check(self._lib.reef_hyrax_create(ctypes.byref(h), self.curve, ptr, n, eb, loc, is_mont, num_vars, self.left,
                                          None if rb is None else rb.ctypes.data, device))
        self._h = h
        self._keep = None

    def _points(self, fn, *args) -> Tuple[np.ndarray, np.ndarray]:
        L, R = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(fn(self._h, *args, L.ctypes.data, R.ctypes.data))
        return L, R

    def eval_begin(self, key: MsmContext, point: Sequence[int], *, is_mont: bool = False) -> Tuple[int, int]:
        """a = LZ, b = eq(point[left..]) on the device; returns (eval, lz_blind).  key: gens_v, exactly 2^right points."""
        if len(point) != self.num_vars:
            raise ValueError(f"expected {self.num_vars} point entries, got {len(point)}")
        pa = _arr(point)
        out = np.zeros((2, 4), dtype=np.uint64)
        check(self._lib.reef_hyrax_eval_begin(self._h, key._h, pa.ctypes.data, is_mont, out[0].ctypes.data, out[1].ctypes.data))
        ev, lb = _ints(out)
        return ev, lb

    def eval_comm(self, row_comms: np.ndarray) -> np.ndarray:
        """comm_LZ = sum_i L_i row_comms[i] (affine (2^left, 8) uint64), Jacobian out"""
        rc = np.ascontiguousarray(row_comms, dtype=np.uint64).reshape(-1, 8)
        if rc.shape[0] != 1 << self.left:
            raise ValueError(f"expected {1 << self.left} row commitments, got {rc.shape[0]}")
        out = np.zeros(12, dtype=np.uint64)
        check(self._lib.reef_hyrax_eval_comm(self._h, rc.ctypes.data, REEF_HOST, out.ctypes.data))
        return out

    def eval_comm_compressed(self, row_comms) -> np.ndarray:
        """comm_LZ from the rows as Reef holds them (PolyCommit.comm): 2^left encodings of 32 bytes -- bytes or a uint8 array (host), or a
        DeviceBuffer -- decoded on the device; Jacobian out.  An invalid row raises ReefError (REEF_ERR_ARG) naming it."""
        want = 32 << self.left
        if isinstance(row_comms, DeviceBuffer):
            if row_comms.nbytes < want:
                raise ValueError(f"expected {want} bytes of row commitments, the device buffer holds {row_comms.nbytes}")
            loc, ptr, keep = REEF_DEVICE, row_comms.ptr, row_comms
        else:
            keep = np.frombuffer(bytes(row_comms), dtype=np.uint8) if isinstance(row_comms, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(row_comms, dtype=np.uint8).reshape(-1)
            if keep.size != want:
                raise ValueError(f"expected {1 << self.left} row commitments of 32 bytes, got {keep.size} bytes")
            loc, ptr = REEF_HOST, keep.ctypes.data
        out = np.zeros(12, dtype=np.uint64)
        check(self._lib.reef_hyrax_eval_comm_compressed(self._h, ptr, loc, out.ctypes.data))
        return out

    def commit(self, key: MsmContext, h: Optional[np.ndarray] = None, *, affine: bool = False):
        """HyraxPC::commit of the resident document: the 2^left row commitments C_i = <Z_i, key> (+ blind_i h) as rows x 32 bytes in
        compress()'s encoding, and with affine=True also as a (2^left, 8) uint64 array.  key: gens_v, exactly 2^right points; h
        (affine, 8 limbs) exactly when the ctx holds row blinds.  The rows stay on the device for eval_comm_own.  Any time after
        creation; an argument in flight is not disturbed."""
        rows = 1 << self.left
        ha = None if h is None else np.ascontiguousarray(h, dtype=np.uint64).reshape(8)
        enc = np.zeros(32 * rows, dtype=np.uint8)
        aff = np.zeros((rows, 8), dtype=np.uint64) if affine else None
        check(self._lib.reef_hyrax_commit(self._h, key._h, None if ha is None else ha.ctypes.data, enc.ctypes.data,
                                          None if aff is None else aff.ctypes.data, REEF_HOST))
        return (enc.tobytes(), aff) if affine else enc.tobytes()

    def commit_to_device(self, key: MsmContext, h: Optional[np.ndarray] = None, comms32: Optional[DeviceBuffer] = None,
                         comms_affine: Optional[DeviceBuffer] = None) -> None:
        """commit with the outputs left in device memory (32 and 64 bytes a row; either or both None: the rows are only kept)"""
        rows = 1 << self.left
        for buf, per in ((comms32, 32), (comms_affine, 64)):
            if buf is not None and buf.nbytes < per * rows:
                raise ValueError(f"{rows} rows of {per} bytes need {per * rows}, the device buffer holds {buf.nbytes}")
        ha = None if h is None else np.ascontiguousarray(h, dtype=np.uint64).reshape(8)
        check(self._lib.reef_hyrax_commit(self._h, key._h, None if ha is None else ha.ctypes.data, None if comms32 is None else comms32.ptr,
                                          None if comms_affine is None else comms_affine.ptr, REEF_DEVICE))

    def eval_comm_own(self) -> np.ndarray:
        """comm_LZ = sum_i L_i C_i over the rows commit() left on the device: no upload; Jacobian out"""
        out = np.zeros(12, dtype=np.uint64)
        check(self._lib.reef_hyrax_eval_comm_own(self._h, out.ctypes.data))
        return out

    def ipa_begin(self, q: np.ndarray, h: Optional[np.ndarray] = None, blinds: Optional[Sequence[int]] = None, *,
                  is_mont: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Round 0's L and R.  q (and h): affine, 8 uint64 limbs in pasta Montgomery coordinates; blinds: round 0's (bl, br)."""
        qa = np.ascontiguousarray(q, dtype=np.uint64).reshape(8)
        ha = None if h is None else np.ascontiguousarray(h, dtype=np.uint64).reshape(8)
        ba = None if blinds is None else _arr(blinds)
        return self._points(self._lib.reef_hyrax_ipa_begin, qa.ctypes.data, None if ha is None else ha.ctypes.data,
                            None if ba is None else ba.ctypes.data, is_mont)

    def ipa_round(self, r: int, blinds: Optional[Sequence[int]] = None, *, is_mont: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        ra = _arr([r])
        ba = None if blinds is None else _arr(blinds)
        return self._points(self._lib.reef_hyrax_ipa_round, ra.ctypes.data, None if ba is None else ba.ctypes.data, is_mont)

    def finish(self, r_last: int, *, is_mont: bool = False) -> Tuple[int, int]:
        """(a_hat, b_hat)"""
        ra = _arr([r_last])
        out = np.zeros((2, 4), dtype=np.uint64)
        check(self._lib.reef_hyrax_finish(self._h, ra.ctypes.data, is_mont, out[0].ctypes.data, out[1].ctypes.data))
        a, b = _ints(out)
        return a, b

    def read(self, which: int, count: int, *, to_mont: bool = False) -> List[int]:
        """which: 0 a, 1 b, as they stand now."""
        out = np.zeros((max(count, 1), 4), dtype=np.uint64)
        check(self._lib.reef_hyrax_read(self._h, which, count, out.ctypes.data, to_mont))
        return _ints(out[:count])

    def set_small_key(self, n_small: int) -> None:
        """The arguments begun (eval_begin) from now on move their rounds to a folded key once a and b have n_small entries
        (reef_hyrax_set_small_key); a power of two, 0: never (the default)."""
        check(self._lib.reef_hyrax_set_small_key(self._h, n_small))


class HyraxBatch(_Handle):
    """The arguments of up to m_max proofs over the resident document of `doc`, advanced in lock-step (include/reef_msm.h 3p): every
    call takes and returns one entry per proof and has one host wait for the whole batch.  The batch borrows doc's document and keeps
    doc alive; an argument in flight on doc itself is not disturbed.  Proof i's outputs are what HyraxEval returns for its point
    alone."""
    _destroy = "reef_hyrax_batch_destroy"

    def __init__(self, doc: HyraxEval, m_max: int):
        self._lib = doc._lib
        self.doc, self.m_max, self.m = doc, m_max, 0
        self.num_vars, self.left, self.right = doc.num_vars, doc.left, doc.right
        h = ctypes.c_void_p()
        check(self._lib.reef_hyrax_batch_create(ctypes.byref(h), doc._h, m_max))
        self._h = h

    def _points(self, fn, *args) -> Tuple[np.ndarray, np.ndarray]:
        L, R = np.zeros((max(self.m, 1), 12), dtype=np.uint64), np.zeros((max(self.m, 1), 12), dtype=np.uint64)
        check(fn(self._h, *args, L.ctypes.data, R.ctypes.data))
        return L[:self.m], R[:self.m]

    def _per_proof(self, vals: Sequence[int], per: int, what: str) -> np.ndarray:
        if len(vals) != per * self.m:
            raise ValueError(f"expected {per * self.m} {what} for {self.m} proofs, got {len(vals)}")
        return _arr(vals) if len(vals) else np.zeros((1, 4), dtype=np.uint64)

    def eval_begin(self, key: MsmContext, points: Sequence[Sequence[int]], *, is_mont: bool = False) -> Tuple[List[int], List[int]]:
        """a_i = LZ_i, b_i = eq(points[i][left..]) on the device; returns (evals, lz_blinds), one entry per point.  Starts the batch
        over with m = len(points) proofs."""
        m = len(points)
        for p in points:
            if len(p) != self.num_vars:
                raise ValueError(f"expected {self.num_vars} point entries, got {len(p)}")
        pa = _arr([x for p in points for x in p]) if m else np.zeros((1, 4), dtype=np.uint64)
        ev, lb = np.zeros((max(m, 1), 4), dtype=np.uint64), np.zeros((max(m, 1), 4), dtype=np.uint64)
        check(self._lib.reef_hyrax_batch_eval_begin(self._h, key._h, pa.ctypes.data, m, is_mont, ev.ctypes.data, lb.ctypes.data))
        if m:
            self.m = m
        return _ints(ev[:m]), _ints(lb[:m])

    def ipa_begin(self, q: np.ndarray, h: Optional[np.ndarray] = None, blinds: Optional[Sequence[int]] = None, *,
                  is_mont: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Round 0's L and R of every proof, (m, 12) each.  q: (m, 8) affine points, one per proof; h: one point for the batch;
        blinds: 2 m entries, (bl, br) of proof 0, of proof 1, ..."""
        qa = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 8)
        if qa.shape[0] != self.m:
            raise ValueError(f"expected {self.m} points q, got {qa.shape[0]}")
        ha = None if h is None else np.ascontiguousarray(h, dtype=np.uint64).reshape(8)
        ba = None if blinds is None else self._per_proof(blinds, 2, "blinds")
        return self._points(self._lib.reef_hyrax_batch_ipa_begin, qa.ctypes.data, None if ha is None else ha.ctypes.data,
                            None if ba is None else ba.ctypes.data, is_mont)

    def ipa_round(self, r: Sequence[int], blinds: Optional[Sequence[int]] = None, *, is_mont: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        ra = self._per_proof(r, 1, "challenges")
        ba = None if blinds is None else self._per_proof(blinds, 2, "blinds")
        return self._points(self._lib.reef_hyrax_batch_ipa_round, ra.ctypes.data, None if ba is None else ba.ctypes.data, is_mont)

    def finish(self, r_last: Sequence[int], *, is_mont: bool = False) -> Tuple[List[int], List[int]]:
        """(a_hats, b_hats), one entry per proof"""
        ra = self._per_proof(r_last, 1, "challenges")
        a, b = np.zeros((max(self.m, 1), 4), dtype=np.uint64), np.zeros((max(self.m, 1), 4), dtype=np.uint64)
        check(self._lib.reef_hyrax_batch_finish(self._h, ra.ctypes.data, is_mont, a.ctypes.data, b.ctypes.data))
        return _ints(a[:self.m]), _ints(b[:self.m])

    def read(self, proof: int, which: int, count: int, *, to_mont: bool = False) -> List[int]:
        """which: 0 a, 1 b of proof `proof`, as they stand now."""
        out = np.zeros((max(count, 1), 4), dtype=np.uint64)
        check(self._lib.reef_hyrax_batch_read(self._h, proof, which, count, out.ctypes.data, to_mont))
        return _ints(out[:count])


def prove_eval(hx: HyraxEval, key: MsmContext, point: Sequence[int], challenge: Callable[[str, List[Any]], int], p: int,
               q_of: Callable[[int], np.ndarray], *, row_comms: Optional[np.ndarray] = None, row_comms_compressed=None,
               h: Optional[np.ndarray] = None,
               blinds_of: Optional[Callable[[int], Tuple[int, int]]] = None, is_mont: bool = False, own_comms: bool = False,
               small_key: Optional[int] = None) -> dict:
    """The whole argument with `challenge(label, absorbed)`: eval_begin, comm_LZ when row_comms (affine) or row_comms_compressed (the
    32-byte rows of PolyCommit.comm, see HyraxEval.eval_comm_compressed) are given or, with own_comms, over the rows
    HyraxEval.commit left on the device, "r" after (comm_LZ, eval)
    for q = q_of(r), then "challenge_r" per round after L and R (compressed).  With h, blinds_of(round) gives that round's (bl, br).
    key: gens_v, exactly 2^right points.  Canonical ints in and out (is_mont: the library calls take Montgomery form)."""
    to, frm = _mont_forms(p, is_mont)
    if small_key is not None:                 # the late rounds on a folded key of that many points (HyraxEval.set_small_key); None: as the ctx stands
        hx.set_small_key(small_key)
    ev, lb = (frm(v) for v in hx.eval_begin(key, [to(x) for x in point], is_mont=is_mont))
    if (row_comms is not None) + (row_comms_compressed is not None) + bool(own_comms) > 1:
        raise ValueError("row_comms, row_comms_compressed or own_comms: one of them")
    comm_lz = hx.eval_comm(row_comms) if row_comms is not None else hx.eval_comm_own() if own_comms else None
    if row_comms_compressed is not None:
        comm_lz = hx.eval_comm_compressed(row_comms_compressed)
    r_ipa = challenge("r", ([compress(key, comm_lz)] if comm_lz is not None else []) + [ev])
    bl = (lambda k: [to(x) for x in blinds_of(k)]) if (h is not None and blinds_of is not None) else (lambda k: None)
    first = hx.ipa_begin(q_of(r_ipa), h if h is not None and blinds_of is not None else None, bl(0), is_mont=is_mont)
    Ls, Rs, rs, (a_hat, b_hat) = _ipa_rounds(first, lambda k, r: hx.ipa_round(to(r), bl(k), is_mont=is_mont),
                                             lambda r: [frm(v) for v in hx.finish(to(r), is_mont=is_mont)], key, challenge, hx.right - 1)
    return {"eval": ev, "lz_blind": lb, "comm_lz": comm_lz, "r_ipa": r_ipa, "L": Ls, "R": Rs, "rs": rs, "a_hat": a_hat, "b_hat": b_hat}


prove = prove_eval   # the argument under the name the other rows use (spartan.prove)
