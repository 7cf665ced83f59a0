"""Python front-end of the sum-checks of the final SNARK (row N5; include/reef_msm.h 3g).

nova-snark's RelaxedR1CSSNARK::prove (Reef: S1 / S2, src/backend/framework.rs:7-8) runs an outer cubic and an inner quadratic
sum-check over the running relaxed instance a `reef_amd.nifs.Nifs` holds on the device.  The transcript stays with the caller:
`prove` drives a whole prove with a caller-supplied `challenge(label, absorbed) -> int` in place of nova's Keccak transcript.
Field elements cross as Python ints: canonical, or pasta Montgomery form with is_mont=True on the `Spartan` methods.

`Opening` is the batched IPA opening that follows on the same ctx (include/reef_msm.h 3h), and `prove_with_opening` runs both.
Points cross as numpy uint64 arrays in the C-ABI layouts: affine (8 limbs) in, Jacobian (12 limbs) out.
"""
from __future__ import annotations

from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from ._fe import _arr, _ints, _mont_forms   # _arr and _ints: importable from here as before
from ._ffi import REEF_HOST, check
from .msm import MsmContext
from .nifs import Nifs


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
    to, frm = _mont_forms(p, is_mont)

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


class Opening:
    """The batched IPA opening on one NIFS ctx after `Spartan.inner_claims`: begin, fold, ipa_begin, ipa_round x (log2(n) - 1),
    finish, with n = max(num_cons_pad, num_vars_pad) and a gens_v key of exactly n points.  Scalars are ints in the caller's form."""

    def __init__(self, nifs: Nifs):
        self.nifs = nifs
        self._lib = nifs._lib

    def _scalar(self, fn, *args) -> int:
        out = np.zeros((1, 4), dtype=np.uint64)
        check(fn(self.nifs._h, *args, out.ctypes.data))
        return _ints(out)[0]

    def _points(self, fn, *args) -> Tuple[np.ndarray, np.ndarray]:
        L, R = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(fn(self.nifs._h, *args, L.ctypes.data, R.ctypes.data))
        return L, R

    def begin(self, key: MsmContext, *, is_mont: bool = False) -> int:
        """The cross term <E, eq(r_y[1..])> + <W, eq(r_x)>."""
        return self._scalar(self._lib.reef_spartan_open_begin, key._h, is_mont)

    def fold(self, r: int, *, is_mont: bool = False) -> int:
        """c = <a, b> after a = E + r W, b = eq(r_x) + r eq(r_y[1..])."""
        ra = _arr([r])
        return self._scalar(self._lib.reef_spartan_open_fold, ra.ctypes.data, is_mont)

    def ipa_begin(self, q: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Round 0's L and R; q: gens_c.scale(r), affine (8 uint64 limbs, pasta Montgomery coordinates)."""
        qa = np.ascontiguousarray(q, dtype=np.uint64).reshape(8)
        return self._points(self._lib.reef_spartan_open_ipa_begin, qa.ctypes.data)

    def ipa_round(self, r: int, *, is_mont: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        ra = _arr([r])
        return self._points(self._lib.reef_spartan_open_ipa_round, ra.ctypes.data, is_mont)

    def finish(self, r_last: int, *, is_mont: bool = False) -> int:
        """a_hat"""
        ra = _arr([r_last])
        return self._scalar(self._lib.reef_spartan_open_finish, ra.ctypes.data, is_mont)

    def read(self, which: int, count: int, *, to_mont: bool = False) -> List[int]:
        """which: 0 a, 1 b, as they stand now."""
        out = np.zeros((max(count, 1), 4), dtype=np.uint64)
        check(self._lib.reef_spartan_open_read(self.nifs._h, which, count, out.ctypes.data, to_mont))
        return _ints(out[:count])

    def set_small_key(self, n_small: int) -> None:
        """The openings begun from now on move their rounds to a folded key once a and b have n_small entries
        (reef_spartan_open_set_small_key); a power of two, 0: never (the default)."""
        check(self._lib.reef_spartan_open_set_small_key(self.nifs._h, n_small))


def compress(key: MsmContext, jac: np.ndarray) -> bytes:
    """A point's 32-byte compressed encoding (what the transcript absorbs), on the device of the library."""
    j = np.ascontiguousarray(jac, dtype=np.uint64).reshape(12)
    out = np.zeros(32, dtype=np.uint8)
    check(key._lib.reef_normalize(key.curve, j.ctypes.data, 1, REEF_HOST, None, out.ctypes.data))
    return out.tobytes()


def _ipa_rounds(first: Tuple[np.ndarray, np.ndarray], step_fn: Callable[[int, int], Tuple[np.ndarray, np.ndarray]], finish_fn: Callable[[int], Any],
                key: MsmContext, challenge: Callable[[str, List[Any]], int], rounds: int) -> Tuple[list, list, List[int], Any]:
    """The IPA rounds of the opening and of the Hyrax argument: "challenge_r" after a round's L and R (compressed), then the next
    round's step_fn(k, r), k = 1..rounds, after round 0's `first`; finish_fn(r) takes the last challenge.  (Ls, Rs, rs, its result)"""
    Ls, Rs, rs = [first[0]], [first[1]], []
    for k in range(rounds):
        rs.append(challenge("challenge_r", [compress(key, Ls[-1]), compress(key, Rs[-1])]))
        L, Rp = step_fn(k + 1, rs[-1])
        Ls.append(L)
        Rs.append(Rp)
    rs.append(challenge("challenge_r", [compress(key, Ls[-1]), compress(key, Rs[-1])]))
    return Ls, Rs, rs, finish_fn(rs[-1])


def prove_with_opening(nifs: Nifs, key: MsmContext, num_cons_pad: int, num_vars_pad: int, challenge: Callable[[str, List[Any]], int],
                       p: int, comm_a: Callable[[int], Any], q_of: Callable[[int], np.ndarray], *, is_mont: bool = False,
                       small_key: Optional[int] = None) -> dict:
    """`prove`, then the batched IPA opening of [E, W] with the same `challenge(label, absorbed)`, in nova's order: "r" (the NIFS
    challenge, after the cross term), "r" again (the IPA's, after comm_a and c), then "challenge_r" per round (after L and R,
    compressed).  The caller's point operations: comm_a(r) = comm_E + r comm_W as the transcript absorbs it, and
    q_of(r) = gens_s.scale(r), affine.  key: gens_v, exactly max(num_cons_pad, num_vars_pad) points.  Canonical ints in and out."""
    out = prove(nifs, num_cons_pad, num_vars_pad, challenge, p, is_mont=is_mont)
    op = Opening(nifs)
    if small_key is not None:                 # the late rounds on a folded key of that many points (Opening.set_small_key); None: as the ctx stands
        op.set_small_key(small_key)
    to, frm = _mont_forms(p, is_mont)
    cross = frm(op.begin(key, is_mont=is_mont))
    r_fold = challenge("r", [cross])
    c = frm(op.fold(to(r_fold), is_mont=is_mont))
    ca = comm_a(r_fold)
    r_ipa = challenge("r", [ca, c])
    n = max(num_cons_pad, num_vars_pad)
    Ls, Rs, rs, a_hat = _ipa_rounds(op.ipa_begin(q_of(r_ipa)), lambda k, r: op.ipa_round(to(r), is_mont=is_mont),
                                    lambda r: frm(op.finish(to(r), is_mont=is_mont)), key, challenge, n.bit_length() - 2)
    out.update({"cross_term": cross, "r_fold": r_fold, "c": c, "comm_a": ca, "r_ipa": r_ipa, "L": Ls, "R": Rs, "r_ipa_rounds": rs,
                "a_hat": a_hat})
    return out
