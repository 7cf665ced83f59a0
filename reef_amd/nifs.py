"""Python front-end of the NIFS fold of one folding step (row N6; include/reef_msm.h 3f).

nova-snark's NIFS::prove (Reef: RecursiveSNARK::prove_step, src/backend/framework.rs:668-675) per curve and step:
the cross term T of the running relaxed instance and a fresh one, comm_T = MSM(T, key), and the folds of W, E, u, X
with the transcript's challenge r.  Vectors are numpy (n, 4) uint64 arrays of canonical limbs (or pasta Montgomery
form with is_mont=True); the matrices are (row, col, value) triples.  All arithmetic runs in libreef_msm.so.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from ._fe import _Handle, _arr
from ._ffi import REEF_DEVICE, REEF_HOST, check
from .msm import DeviceBuffer, MsmContext, curve_id

W, E, T, U, X = 0, 1, 2, 3, 4          # reef_nifs_read: which
A, B, C = 0, 1, 2                      # reef_nifs_set_matrix: which


def _fe(arr, n: Optional[int] = None) -> np.ndarray:
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"expected {n} field elements, got {a.shape[0]}")
    return a


def _fe_in(arr, n: int):
    """(loc, address, keep-alive) of n field elements: an array of canonical limbs, or a DeviceBuffer of exactly that many."""
    if isinstance(arr, DeviceBuffer):
        if arr.nbytes != 32 * n:
            raise ValueError(f"expected {n} field elements, the device buffer holds {arr.nbytes // 32}")
        return REEF_DEVICE, arr.ptr, arr
    a = _fe(arr, n)
    return REEF_HOST, a.ctypes.data, a


class Nifs(_Handle):
    """The resident running instance, the fresh witness and T of one R1CS shape over the scalar field of `curve`."""
    _destroy = "reef_nifs_destroy"

    def __init__(self, curve, num_cons: int, num_vars: int, num_io: int, device: int = 0):
        self._lib = _ffi.load()
        self.curve = curve_id(curve)
        self.num_cons, self.num_vars, self.num_io = num_cons, num_vars, num_io
        h = ctypes.c_void_p()
        check(self._lib.reef_nifs_create(ctypes.byref(h), self.curve, num_cons, num_vars, num_io, device))
        self._h = h

    def set_matrix(self, which: int, rows, cols, vals, *, is_mont: bool = False) -> None:
        """Matrix A, B or C from (row, col, value) triples in any order; duplicates are summed."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        c = np.ascontiguousarray(cols, dtype=np.uint32)
        v = _fe(vals, r.shape[0])
        if c.shape[0] != r.shape[0]:
            raise ValueError("rows and cols differ in length")
        check(self._lib.reef_nifs_set_matrix(self._h, which, r.ctypes.data, c.ctypes.data, v.ctypes.data, r.shape[0], is_mont))

    def set_running(self, w, e, u, x, *, is_mont: bool = False) -> None:
        """The running relaxed instance (W, E, u, X); e=None: E = 0 (nova's first step, with u = 1)."""
        wa, ua, xa = _fe(w, self.num_vars), _fe(u, 1), _fe(x, self.num_io)
        ea = None if e is None else _fe(e, self.num_cons)
        check(self._lib.reef_nifs_set_running(self._h, wa.ctypes.data, None if ea is None else ea.ctypes.data, ua.ctypes.data,
                                              xa.ctypes.data, REEF_HOST, is_mont))

    def commit_t(self, key: MsmContext, w2, x2, *, is_mont: bool = False) -> np.ndarray:
        """T of the running and the fresh instance (W2, 1, X2) on the device; returns comm_T (uint64[12] Jacobian)."""
        wa, xa = _fe(w2, self.num_vars), _fe(x2, self.num_io)
        out = np.zeros(12, dtype=np.uint64)
        check(self._lib.reef_nifs_commit_T(self._h, key._h, wa.ctypes.data, xa.ctypes.data, REEF_HOST, is_mont, out.ctypes.data))
        return out

    def commit_step(self, key: MsmContext, w2, x2, *, is_mont: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """commit_t and the fresh witness's commitment from one upload of w2: (comm_W2, comm_T), uint64[12] Jacobian each, no blinds.
        w2 and x2 are arrays, or DeviceBuffers (both of one kind)."""
        wloc, wp, _wk = _fe_in(w2, self.num_vars)
        xloc, xp, _xk = _fe_in(x2, self.num_io)
        if wloc != xloc:
            raise ValueError("w2 and x2 must both be host arrays or both DeviceBuffers")
        cw, ct = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(self._lib.reef_nifs_commit_step(self._h, key._h, wp, xp, wloc, is_mont, cw.ctypes.data, ct.ctypes.data))
        return cw, ct

    def commit_running(self, key: MsmContext) -> Tuple[np.ndarray, np.ndarray]:
        """(comm_W, comm_E) of the running instance as it stands, uint64[12] Jacobian each, no blinds; reads only."""
        cw, ce = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(self._lib.reef_nifs_commit_running(self._h, key._h, cw.ctypes.data, ce.ctypes.data))
        return cw, ce

    def check_fresh(self) -> Tuple[int, Optional[int]]:
        """(rows of the last fresh instance (W2, 1, X2) violating AZ o BZ == CZ, the first of them or None)."""
        v, f = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._lib.reef_nifs_check_fresh(self._h, ctypes.byref(v), ctypes.byref(f)))
        return v.value, (None if v.value == 0 else f.value)

    def fold(self, r: int, *, is_mont: bool = False) -> None:
        """W, E, u, X of the running instance folded with the last commit_t's / commit_step's fresh instance and T."""
        ra = _arr([r])
        check(self._lib.reef_nifs_fold(self._h, ra.ctypes.data, is_mont))

    def read(self, which: int, count: Optional[int] = None, *, to_mont: bool = False) -> np.ndarray:
        if count is None:
            count = {W: self.num_vars, E: self.num_cons, T: self.num_cons, U: 1, X: self.num_io}[which]
        out = np.zeros((count, 4), dtype=np.uint64)
        check(self._lib.reef_nifs_read(self._h, which, count, out.ctypes.data, to_mont))
        return out

    def check_relaxed(self) -> Tuple[int, Optional[int]]:
        """(rows violating AZ o BZ == u CZ + E, the first of them or None)."""
        v, f = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._lib.reef_nifs_check_relaxed(self._h, ctypes.byref(v), ctypes.byref(f)))
        return v.value, (None if v.value == 0 else f.value)

    def set_eval_workspace(self, nbytes: int) -> None:
        """The budget of the eq tables a `verify.matrix_evals_batch` call may hold (reef_nifs_set_eval_workspace): the batch walks its
        points in groups whose tables fit it.  0: the default of 1 GiB.  A budget below one point's tables gives groups of one."""
        check(self._lib.reef_nifs_set_eval_workspace(self._h, nbytes))

    def eval_batch_last_info(self) -> dict:
        """How the last `verify.matrix_evals_batch` on this ctx divided (reef_spartan_eval_matrices_batch_last_info): "groups",
        "points_per_group" and "workspace_bytes" (the tables' buffer as it stands).  ReefError when there was no batch."""
        g, k, b = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        check(self._lib.reef_spartan_eval_matrices_batch_last_info(self._h, ctypes.byref(g), ctypes.byref(k), ctypes.byref(b)))
        return {"groups": g.value, "points_per_group": k.value, "workspace_bytes": b.value}
