"""Python front-end of the sum-checks of the final SNARK (row N5; include/reef_msm.h 3g).

nova-snark's RelaxedR1CSSNARK::prove (Reef: S1 / S2, src/backend/framework.rs:7-8) runs an outer cubic and an inner quadratic
sum-check over the running relaxed instance a `reef_amd.nifs.Nifs` holds on the device.  The transcript stays with the caller:
`prove` drives a whole prove with a caller-supplied `challenge(label, absorbed) -> int` in place of nova's Keccak transcript.
Field elements cross as Python ints: canonical, or pasta Montgomery form with is_mont=True on the `Spartan` methods.
"""
from __future__ import annotations

from typing import Callable, List, Sequence

import numpy as np

from ._ffi import check
from .nifs import Nifs


def _arr(vals: Sequence[int]) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def _ints(a: np.ndarray) -> List[int]:
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


class Spartan:
    """The prover-side state machine on one NIFS ctx: begin, outer_round x (log2(num_cons_pad) - 1), outer_claims, inner_begin,
    inner_round x log2(num_vars_pad), inner_claims.  Values are ints in the caller's form (is_mont)."""

    def __init__(self, nifs: Nifs):
        self.nifs = nifs
        self._lib = nifs._lib

    def _call(self, fn, r: int, n_out: int, is_mont: bool) -> List[int]:
        ra = _arr([r])
        out = np.zeros((n_out, 4), dtype=np.uint64)
        check(fn(self.nifs._h, ra.ctypes.data, is_mont, out.ctypes.data))
        return _ints(out)

    def begin(self, num_cons_pad: int, num_vars_pad: int, tau: Sequence[int], *, is_mont: bool = False) -> List[int]:
        """Round 0 of the outer sum-check: [e0, e2, e3]."""
        ta = _arr(tau) if len(tau) else np.zeros((1, 4), dtype=np.uint64)
        out = np.zeros((3, 4), dtype=np.uint64)
        check(self._lib.reef_spartan_begin(self.nifs._h, num_cons_pad, num_vars_pad, ta.ctypes.data, is_mont, out.ctypes.data))
        return _ints(out)

    def outer_round(self, r: int, *, is_mont: bool = False) -> List[int]:
        return self._call(self._lib.reef_spartan_outer_round, r, 3, is_mont)

    def outer_claims(self, r_last: int, *, is_mont: bool = False) -> List[int]:
        """[AZ(r_x), BZ(r_x), CZ(r_x), E(r_x)]"""
        return self._call(self._lib.reef_spartan_outer_claims, r_last, 4, is_mont)

    def inner_begin(self, r: int, *, is_mont: bool = False) -> List[int]:
        """Round 0 of the inner sum-check: [e0, e2]."""
        return self._call(self._lib.reef_spartan_inner_begin, r, 2, is_mont)

    def inner_round(self, r: int, *, is_mont: bool = False) -> List[int]:
        return self._call(self._lib.reef_spartan_inner_round, r, 2, is_mont)

    def inner_claims(self, r_last: int, *, is_mont: bool = False) -> List[int]:
        """[ABC(r_y), z(r_y), eval_W]"""
        return self._call(self._lib.reef_spartan_inner_claims, r_last, 3, is_mont)


def prove(nifs: Nifs, num_cons_pad: int, num_vars_pad: int, challenge: Callable[[str, List[int]], int], p: int, *,
          is_mont: bool = False) -> dict:
    """One whole prove of both sum-checks, challenges from `challenge(label, absorbed)` in nova's order: "t" (tau, one per
    outer round, nothing absorbed), "outer" (a round's [e0, e2, e3]), "r" (the four outer claims), "inner" (a round's [e0, e2]).
    p: the scalar field's modulus.  Canonical ints in and out; is_mont only chooses the form the library is called with."""
    sp = Spartan(nifs)
    R = (1 << 256) % p
    Rinv = pow(R, -1, p)
    to = (lambda v: v * R % p) if is_mont else (lambda v: v)
    frm = (lambda v: v * Rinv % p) if is_mont else (lambda v: v)

    def run(fn, *a):
        return [frm(v) for v in fn(*a, is_mont=is_mont)]

    ell_x = num_cons_pad.bit_length() - 1
    ell_y = (2 * num_vars_pad).bit_length() - 1
    tau = [challenge("t", []) for _ in range(ell_x)]
    outer, r_x = [run(sp.begin, num_cons_pad, num_vars_pad, [to(t) for t in tau])], []
    for _ in range(ell_x - 1):
        r_x.append(challenge("outer", outer[-1]))
        outer.append(run(sp.outer_round, to(r_x[-1])))
    r_x.append(challenge("outer", outer[-1]))
    claims_outer = run(sp.outer_claims, to(r_x[-1]))
    r = challenge("r", claims_outer)
    inner, r_y = [run(sp.inner_begin, to(r))], []
    for _ in range(ell_y - 1):
        r_y.append(challenge("inner", inner[-1]))
        inner.append(run(sp.inner_round, to(r_y[-1])))
    r_y.append(challenge("inner", inner[-1]))
    claims_inner = run(sp.inner_claims, to(r_y[-1]))
    return {"tau": tau, "outer": outer, "r_x": r_x, "claims_outer": claims_outer, "r": r, "inner": inner, "r_y": r_y,
            "claims_inner": claims_inner}
