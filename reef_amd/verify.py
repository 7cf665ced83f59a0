"""Python front-end of the verifier's device calls: the IPA check (include/reef_msm.h 3j) and the matrix evaluations (3k).

`ipa_check` / `ipa_check_eq` are the two C-ABI calls: P_hat rebuilt from the proof, the challenges expanded into s on the device,
G_hat = <s, key>, b_hat = <s, b>, and the two sides compared as group elements.  `verify_opening` is the device counterpart of
EE::verify_batch at the end of CompressedSNARK::verify (3h's opening), `verify_eval` of HyraxPC::verify_eval inside
verify_consistency (3i's argument); both take a caller-supplied `challenge(label, absorbed) -> int` in place of the transcript and
draw their challenges in the provers' label order.  A proof that does not verify gives False, never an exception; bad arguments
raise ReefError (REEF_ERR_ARG).  The C calls take no curve -- the key's curve is the call's -- so "a key of another curve" is a
check of THIS module, not of the library: pass curve= and a key of another curve raises ReefError(1) before any call is made.
Scalars cross as Python ints (canonical, or pasta Montgomery form with is_mont=True); points as numpy uint64 arrays in the C-ABI
layouts: affine (8 limbs) or Jacobian (12 limbs).

`ipa_check_batch` is reef_ipa_check_batch (3m): m proofs over the same n against the one key under caller-drawn weights rho -- one MSM
over the key whatever m is; `verify_eval_batch` drives m Hyrax arguments through it the way `verify_eval` drives one.  The weights
are the caller's randomness, drawn after every proof is fixed; neither function draws any.

`HyraxVk` is the verifier's key of a committed document (3n): the row commitments decoded and keyed once, `.comm_lz(points)` then
forms comm_LZ for any number of points in one call.  An instance of `verify_eval` / `verify_eval_batch` may carry one in place of
its rows; the batch makes one call per vk and takes the transcript's encodings from it.

`matrix_evals` is reef_spartan_eval_matrices: A~, B~, C~ at (r_x, r_y) on the matrices a `Nifs` holds, no witness needed.
`verify_sumchecks` is the verifier of 3g's transcript -- RelaxedR1CSSNARK::verify [R] up to the opening: O(log n) host arithmetic and that
one device call -- and `verify_snark` adds `verify_opening` with eval_E = claims_outer[3], eval_W = claims_inner[2].
`matrix_evals_batch` is reef_spartan_eval_matrices_batch (3o): the same three values at many points in one call, and
`verify_sumchecks_batch` verifies many proofs over one shape with one such call.
"""
from __future__ import annotations

import ctypes
from typing import Any, Callable, List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import REEF_DEVICE, REEF_HOST, IpaProof, MsmOpts, ReefError, check
from ._fe import _Handle, _arr, _ints
from .msm import DeviceBuffer, MsmContext, curve_id, decompress, normalize
from .nifs import Nifs
from .spartan import compress


def _jac(pts, count: Optional[int] = None) -> np.ndarray:
    a = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.uint64).reshape(12) for x in pts]) if isinstance(pts, (list, tuple)) else pts,
                             dtype=np.uint64).reshape(-1, 12)
    if count is not None and a.shape[0] != count:
        raise ValueError(f"expected {count} points, got {a.shape[0]}")
    return a


def _aff(pt) -> np.ndarray:
    return np.ascontiguousarray(pt, dtype=np.uint64).reshape(8)


def _rounds(n: int) -> int:
    return max(n.bit_length() - 1, 0)


def _call(key: MsmContext, fn, n, comm, c, q, L, R, rs, a_hat, mid, h, blind, is_mont, intermediates, curve):
    if curve is not None and curve_id(curve) != key.curve:
        raise ReefError(1, f"the key is of curve {key.curve}, the check of curve {curve_id(curve)}")
    k = _rounds(n)
    ca, qa = _jac([comm], 1), _aff(q)
    if (len(rs) != k or len(L) != k or len(R) != k) and n >= 2 and n & (n - 1) == 0:
        raise ValueError(f"n = {n} takes {k} rounds: L, R and rs have {len(L)}, {len(R)}, {len(rs)} entries")
    if not (len(L) and len(R) and len(rs)):
        L, R, rs = [np.zeros(12, np.uint64)], [np.zeros(12, np.uint64)], [0]      # n < 2: the library says what is wrong with it
    La, Ra = _jac(L, len(L)), _jac(R, len(R))
    cs, rsa, aa = _arr([c]), _arr(rs), _arr([a_hat])
    ha = None if h is None else _aff(h)
    ba = None if blind is None else _arr([blind])
    accept = ctypes.c_uint32(0xFFFFFFFF)
    ph, gh, bh = (np.zeros(12, np.uint64), np.zeros(12, np.uint64), np.zeros((1, 4), np.uint64)) if intermediates else (None, None, None)
    check(fn(key._h, n, ca.ctypes.data, cs.ctypes.data, qa.ctypes.data, La.ctypes.data, Ra.ctypes.data, rsa.ctypes.data, aa.ctypes.data,
             *mid, None if ha is None else ha.ctypes.data, None if ba is None else ba.ctypes.data, bool(is_mont), ctypes.byref(accept),
             None if ph is None else ph.ctypes.data, None if gh is None else gh.ctypes.data, None if bh is None else bh.ctypes.data))
    out = {"accept": accept.value == 1}
    if intermediates:
        out.update({"p_hat": ph, "g_hat": gh, "b_hat": _ints(bh)[0]})
    return out


def ipa_check(key: MsmContext, n: int, comm, c: int, q, L, R, rs: Sequence[int], a_hat: int, b, *, b_len: Optional[int] = None, h=None,
              blind: Optional[int] = None, is_mont: bool = False, intermediates: bool = False, curve=None) -> dict:
    """reef_ipa_check.  b: ints (at most n of them; the rest is zero padding), or a DeviceBuffer of b_len field elements in the form
    is_mont names.  {"accept": bool} and, with intermediates, "p_hat", "g_hat" (Jacobian) and "b_hat"."""
    if isinstance(b, DeviceBuffer):
        if b_len is None or b.nbytes < 32 * b_len:
            raise ValueError("a device b needs b_len, and 32 bytes per entry")
        mid, keep = (b.ptr, b_len, REEF_DEVICE), b
    else:
        keep = _arr(b) if len(b) else np.zeros((1, 4), np.uint64)
        mid = (keep.ctypes.data if len(b) else None, len(b), REEF_HOST)
    return _call(key, key._lib.reef_ipa_check, n, comm, c, q, L, R, rs, a_hat, mid, h, blind, is_mont, intermediates, curve)


def ipa_check_eq(key: MsmContext, n: int, comm, c: int, q, L, R, rs: Sequence[int], a_hat: int, points: Sequence[Sequence[int]],
                 weights: Sequence[int], *, h=None, blind: Optional[int] = None, is_mont: bool = False, intermediates: bool = False,
                 curve=None) -> dict:
    """reef_ipa_check_eq: b = sum_t weights[t] pad(eq(points[t])) built on the device, one or two points."""
    if len(points) != len(weights):
        raise ValueError("one weight per point")
    arrs = [_arr(pt) if len(pt) else np.zeros((1, 4), np.uint64) for pt in points]
    ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    nvars = (ctypes.c_size_t * max(len(arrs), 1))(*[len(pt) for pt in points])
    wa = _arr(weights) if len(weights) else np.zeros((1, 4), np.uint64)
    mid = (ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nvars, ctypes.c_void_p), wa.ctypes.data, len(points))
    return _call(key, key._lib.reef_ipa_check_eq, n, comm, c, q, L, R, rs, a_hat, mid, h, blind, is_mont, intermediates, curve)


def eq_b_hat(rs: Sequence[int], points: Sequence[Sequence[int]], weights: Sequence[int], p: int) -> int:
    """<s, b> for b = sum_t weights[t] pad(eq(points[t])) in O(k) products per point, as reef_ipa_check_batch forms it on the host:
    with v = len(points[t]), prod_{i < k - v} rs[i]^-1 prod_{j < v} ((1 - p_j) rs[k-v+j]^-1 + p_j rs[k-v+j]).  Canonical ints."""
    k = len(rs)
    inv = [pow(r, -1, p) for r in rs]
    out = 0
    for pt, w in zip(points, weights):
        v = len(pt)
        if v > k:
            raise ValueError(f"a point of {v} variables against {k} rounds")
        acc = 1
        for i in range(k - v):
            acc = acc * inv[i] % p
        for j, x in enumerate(pt):
            acc = acc * ((1 - x) * inv[k - v + j] + x * rs[k - v + j]) % p
        out = (out + w * acc) % p
    return out


def _marshal_batch(n: int, proofs: Sequence[dict], rho: Sequence[int]):
    """(reef_ipa_proof array, rho array, what must stay alive until the call returns)"""
    m = len(proofs)
    k = _rounds(n)
    pow2 = n >= 2 and n & (n - 1) == 0
    structs = (IpaProof * max(m, 1))()
    keep = []
    for i, pr in enumerate(proofs):
        L, R, rs = pr["L"], pr["R"], pr["rs"]
        if pow2 and (len(rs) != k or len(L) != k or len(R) != k):
            raise ValueError(f"proof {i}: n = {n} takes {k} rounds: L, R and rs have {len(L)}, {len(R)}, {len(rs)} entries")
        if not (len(L) and len(R) and len(rs)):
            L, R, rs = [np.zeros(12, np.uint64)], [np.zeros(12, np.uint64)], [0]  # n < 2: the library says what is wrong with it
        points, weights = pr["points"], pr["weights"]
        if len(points) != len(weights):
            raise ValueError(f"proof {i}: one weight per point")
        arrs = [_arr(pt) if len(pt) else np.zeros((1, 4), np.uint64) for pt in points]
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        nvars = (ctypes.c_size_t * max(len(arrs), 1))(*[len(pt) for pt in points])
        wa = _arr(weights) if len(weights) else np.zeros((1, 4), np.uint64)
        own = [_jac([pr["comm"]], 1), _arr([pr["c"]]), _aff(pr["q"]), _jac(L, len(L)), _jac(R, len(R)), _arr(rs), _arr([pr["a_hat"]]), wa]
        ha = None if pr.get("h") is None else _aff(pr["h"])
        ba = None if pr.get("blind") is None else _arr([pr["blind"]])
        keep.append((own, arrs, ptrs, nvars, ha, ba))
        s = structs[i]
        s.comm, s.c, s.q, s.L, s.R, s.rs, s.a_hat, s.weights = (a.ctypes.data for a in own)
        s.points, s.vars, s.npoints = ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nvars, ctypes.c_void_p), len(points)
        s.h, s.blind = None if ha is None else ha.ctypes.data, None if ba is None else ba.ctypes.data
    ra = _arr(rho) if m else np.zeros((1, 4), np.uint64)
    return structs, ra, keep


def ipa_check_batch(key: MsmContext, n: int, proofs: Sequence[dict], rho: Sequence[int], *, is_mont: bool = False, each: bool = False,
                    intermediates: bool = False, s_comb_out: Optional[DeviceBuffer] = None, curve=None) -> dict:
    """reef_ipa_check_batch: m proofs over the same n against `key` in one pass.  proofs: dicts with the arguments of `ipa_check_eq`
    ("comm", "c", "q", "L", "R", "rs", "a_hat", "points", "weights" and, for a blinded one, "h" and "blind").  rho: one non-zero weight
    per proof, the CALLER'S randomness, drawn after all the proofs are fixed.  {"accept": bool}; with each, "each": a bool per proof
    (the single checks run only when the batch rejects); with intermediates, "b_hats" (ints), "s_comb" (n ints, canonical),
    "d_comb" and "g_comb" (Jacobian): the two sides of the combined equation.  s_comb_out: a DeviceBuffer of 32 n bytes that takes S
    instead of the host."""
    if curve is not None and curve_id(curve) != key.curve:
        raise ReefError(1, f"the key is of curve {key.curve}, the check of curve {curve_id(curve)}")
    m = len(proofs)
    if len(rho) != m:
        raise ValueError("one weight per proof")
    structs, ra, keep = _marshal_batch(n, proofs, rho)
    accept = ctypes.c_uint32(0xFFFFFFFF)
    ea = (ctypes.c_uint32 * max(m, 1))(*([0xFFFFFFFF] * max(m, 1))) if each else None
    bh = np.zeros((max(m, 1), 4), np.uint64) if intermediates else None
    dc, gc = (np.zeros(12, np.uint64), np.zeros(12, np.uint64)) if intermediates else (None, None)
    sc, s_ptr, s_loc = None, None, REEF_HOST
    if s_comb_out is not None:
        if s_comb_out.nbytes < 32 * n:
            raise ValueError("s_comb_out needs 32 bytes per entry")
        s_ptr, s_loc = s_comb_out.ptr, REEF_DEVICE
    elif intermediates:
        sc = np.zeros((max(n, 1), 4), np.uint64)
        s_ptr = sc.ctypes.data
    check(key._lib.reef_ipa_check_batch(key._h, n, structs, m, ra.ctypes.data, bool(is_mont), ctypes.byref(accept),
                                        None if ea is None else ctypes.cast(ea, ctypes.c_void_p), None if bh is None else bh.ctypes.data, s_ptr, s_loc,
                                        None if dc is None else dc.ctypes.data, None if gc is None else gc.ctypes.data))
    out = {"accept": accept.value == 1}
    if each:
        out["each"] = [ea[i] == 1 for i in range(m)]
    if intermediates:
        out.update({"b_hats": _ints(bh)[:m], "d_comb": dc, "g_comb": gc})
        if sc is not None:
            out["s_comb"] = _ints(sc)[:n]
    return out


def ipa_check_batch_timing(key: MsmContext) -> dict:
    """reef_ipa_check_batch_last_timing: device milliseconds of the last batch on `key`, run with key.enable_timing() on."""
    s, g, d = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    check(key._lib.reef_ipa_check_batch_last_timing(key._h, ctypes.byref(s), ctypes.byref(g), ctypes.byref(d)))
    return {"s_pass_ms": s.value, "key_msm_ms": g.value, "side_ms": d.value}


def _lincomb(curve: int, points, scalars: Sequence[int]) -> np.ndarray:
    """sum scalars[i] points[i] through calls that exist: reef_normalize, a plain key, reef_msm.  Jacobian (12) or affine (8) in,
    Jacobian out"""
    aff = []
    for pt in points:
        a = np.ascontiguousarray(pt, dtype=np.uint64).reshape(-1)
        aff.append(a if a.size == 8 else normalize(curve, a)[0][0])
    with MsmContext(curve, np.stack(aff), byte_tables=2) as ctx:
        return ctx.msm(_arr(scalars), is_mont=False)


def verify_opening(key: MsmContext, gens_s, comm_e, r_x: Sequence[int], eval_e: int, comm_w, r_y: Sequence[int], eval_w: int, proof: dict,
                   challenge: Callable[[str, List[Any]], int], p: int, *, check_fn=None) -> bool:
    """EE::verify_batch [R] over the instances [E, W] of 3h: {comm_E, eq(r_x), eval_E} and {comm_W, eq(r_y[1..]), eval_W}, and the
    proof {"cross", "L", "R", "a_hat"}.  Challenges: "r" after the cross term, "r" after (comm_a, c), "challenge_r" per round after
    (L, R) compressed -- prove_with_opening's order.  key: gens_v with at least n = max(2^len(r_x), 2^(len(r_y) - 1)) points; gens_s:
    one affine point.  Canonical ints.  check_fn: stands in for ipa_check_eq (tests)."""
    curve = key.curve
    ry = list(r_y[1:])
    n = max(1 << len(r_x), 1 << len(ry))
    r = challenge("r", [proof["cross"]])
    c = (eval_e + r * r * eval_w + r * proof["cross"]) % p
    comm_a = _lincomb(curve, [comm_e, comm_w], [1, r])
    r_ipa = challenge("r", [compress(key, comm_a), c])
    q = normalize(curve, _lincomb(curve, [gens_s], [r_ipa]))[0][0]
    if len(proof["L"]) != _rounds(n) or len(proof["R"]) != _rounds(n):
        return False
    rs = [challenge("challenge_r", [compress(key, L), compress(key, R)]) for L, R in zip(proof["L"], proof["R"])]
    fn = check_fn or ipa_check_eq
    return fn(key, n, comm_a, c, q, proof["L"], proof["R"], rs, proof["a_hat"], [list(r_x), ry], [1, r])["accept"]


def comm_lz(curve, row_comms32, point_left: Sequence[int], p: int) -> np.ndarray:
    """comm_LZ = sum_i eq(point[..left])_i C_i from the 32-byte rows a .cmt file holds, without a document: reef_decompress to device
    memory, reef_msm_ctx_set_bases on a plain context, reef_msm with the weights built on the host (2^left of them)."""
    rows = 1 << len(point_left)
    enc = np.frombuffer(bytes(row_comms32), dtype=np.uint8) if isinstance(row_comms32, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(row_comms32, dtype=np.uint8).reshape(-1)
    if enc.size != 32 * rows:
        raise ValueError(f"expected {rows} row commitments of 32 bytes, got {enc.size} bytes")
    dec, bad, first = decompress(curve, DeviceBuffer.from_host(enc), rows)
    if bad:
        raise ReefError(1, f"row {first} is not the encoding of a point ({bad} such rows)")
    w = [1]
    for x in point_left:
        w = [v for e in w for v in (e * (1 - x) % p, e * x % p)]
    with MsmContext(curve, np.zeros((1, 8), np.uint64), byte_tables=2) as ctx:
        ctx.set_bases(dec, rows)
        return ctx.msm(_arr(w), is_mont=False)


class HyraxVk(_Handle):
    """reef_hyrax_vk (3n): the verifier's key of a committed document.  row_comms32: the 2^left rows of 32 bytes a .cmt file holds
    (bytes or a uint8 array), or a DeviceBuffer of them; decoded and keyed once, on `device` (None: the current one).  The keyword
    options are MsmContext's (the default: the library's default key)."""
    _destroy = "reef_hyrax_vk_destroy"

    def __init__(self, curve, row_comms32, left: int, *, device: Optional[int] = None, window_bits: int = 0, bucket_groups: int = 0,
                 chunk: int = 0, byte_tables: int = 0):
        self.curve = curve_id(curve)
        self.left = int(left)
        self._lib = _ffi.load()
        self._h = None
        if not 1 <= self.left <= 25:
            raise ReefError(1, f"left_vars = {self.left} is outside 1 .. 25")
        nbytes = 32 << self.left
        if isinstance(row_comms32, DeviceBuffer):
            if row_comms32.nbytes < nbytes:
                raise ValueError(f"expected {1 << self.left} row commitments of 32 bytes, the device buffer holds {row_comms32.nbytes} bytes")
            loc, ptr, keep = REEF_DEVICE, row_comms32.ptr, row_comms32
        else:
            keep = np.frombuffer(bytes(row_comms32), dtype=np.uint8) if isinstance(row_comms32, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(row_comms32, dtype=np.uint8).reshape(-1)
            if keep.size != nbytes:
                raise ValueError(f"expected {1 << self.left} row commitments of 32 bytes, got {keep.size} bytes")
            loc, ptr = REEF_HOST, keep.ctypes.data
        opts = MsmOpts(window_bits, bucket_groups, chunk, byte_tables, -1, (ctypes.c_uint32 * 3)(0, 0, 0))
        h = ctypes.c_void_p()
        check(self._lib.reef_hyrax_vk_create(ctypes.byref(h), self.curve, ptr, self.left, loc, -1 if device is None else int(device),
                                             ctypes.byref(opts)))
        self._h = h

    def comm_lz(self, points: Sequence[Sequence[int]], compressed: bool = True, *, is_mont: bool = False):
        """reef_hyrax_vk_comm_lz: comm_LZ for every point (each `left` ints in the form is_mont names) in one call.  (jacobians,
        encodings): an (m, 12) uint64 array and a list of m 32-byte strings (None unless compressed)."""
        m = len(points)
        for t, pt in enumerate(points):
            if len(pt) != self.left:
                raise ValueError(f"point {t} has {len(pt)} entries, the key is over 2^{self.left} rows")
        jac = np.zeros((m, 12), np.uint64)
        enc = np.zeros((m, 32), np.uint8) if compressed else None
        if m:
            pa = _arr([x for pt in points for x in pt])
            check(self._lib.reef_hyrax_vk_comm_lz(self._h, pa.ctypes.data, m, bool(is_mont), jac.ctypes.data,
                                                  None if enc is None else enc.ctypes.data))
        return jac, (None if enc is None else [enc[t].tobytes() for t in range(m)])


def _check_vk(vk: "HyraxVk", curve: int, left: int, who: str, i: Optional[int] = None) -> None:
    where = "" if i is None else f"instance {i}: "
    if vk.curve != curve:
        raise ReefError(1, f"{who}: {where}the vk is of curve {vk.curve}, the key of curve {curve}")
    if vk.left != left:
        raise ValueError(f"{who}: {where}the vk is over 2^{vk.left} rows, the instance has left = {left}")


def verify_eval(key: MsmContext, q, row_comms32, point: Sequence[int], left: int, eval_: int, proof: dict, p: int, *, h=None,
                blind_total: Optional[int] = None, challenge: Optional[Callable[[str, List[Any]], int]] = None, q_of=None,
                check_fn=None) -> bool:
    """HyraxPC::verify_eval [R] for 3i's argument: comm_LZ from the compressed row commitments (comm_lz above), then P_hat = comm_LZ +
    eval q + sum r_k^2 L_k + sum r_k^-2 R_k against a_hat G_hat + a_hat b_hat q (+ blind_total h), b = eq(point[left..]) built on the
    device.  proof: {"L", "R", "a_hat"} and either "rs", or a `challenge` to draw them with: "r" after (comm_LZ, eval) -- q is then
    q_of(r) -- and "challenge_r" per round, prove_eval's order.  key: gens_v with 2^(len(point) - left) points.  Canonical ints.
    row_comms32 may be a `HyraxVk` over the rows instead: comm_LZ and its encoding then come from the vk."""
    curve = key.curve
    right = len(point) - left
    n = 1 << right
    if challenge is None and "rs" not in proof:
        raise ValueError("verify_eval needs the round challenges: proof['rs'], or a challenge callable to draw them")
    if q is None and (challenge is None or q_of is None):
        raise ValueError("verify_eval needs q, or a challenge callable and q_of to form it from the drawn r")
    if (h is None) != (blind_total is None):
        raise ValueError("h and blind_total come together or not at all")
    if isinstance(row_comms32, HyraxVk):
        _check_vk(row_comms32, curve, left, "verify_eval")
        jac, encs = row_comms32.comm_lz([[x % p for x in point[:left]]])
        clz, cz = jac[0], encs[0]
    else:
        clz, cz = comm_lz(curve, row_comms32, point[:left], p), None
    if challenge is not None:
        r_ipa = challenge("r", [compress(key, clz) if cz is None else cz, eval_])
        if q_of is not None:
            q = q_of(r_ipa)
        rs = [challenge("challenge_r", [compress(key, L), compress(key, R)]) for L, R in zip(proof["L"], proof["R"])]
    else:
        rs = list(proof["rs"])
    if len(proof["L"]) != right or len(proof["R"]) != right or len(rs) != right:
        return False
    fn = check_fn or ipa_check_eq
    blind = None if blind_total is None else blind_total % p
    return fn(key, n, clz, eval_ % p, q, proof["L"], proof["R"], rs, proof["a_hat"], [list(point[left:])], [1], h=h, blind=blind)["accept"]


def verify_eval_batch(key: MsmContext, instances: Sequence[dict], p: int, weights: Callable[[List[List[Any]]], Sequence[int]], *,
                      each: bool = False, check_fn=None):
    """m Hyrax arguments over the same gens_v checked in one pass: `verify_eval` for each instance up to its IPA check, then one
    `ipa_check_batch`.  instances: dicts with verify_eval's arguments -- "q", "row_comms32", "point", "left", "eval", "proof" and,
    where used, "h", "blind_total", "challenge", "q_of" -- all with the same len(point) - left.  weights(absorbed) -> m non-zero ints
    below p: the caller's randomness, called once AFTER every proof is fixed, with what each proof contributes ([comm_LZ compressed,
    eval, a_hat, L and R compressed ...] per instance) for a caller that derives the weights from a transcript.  True / False; with
    each, (verdict, [bool per instance]).  check_fn stands in for ipa_check_batch (tests).
    An instance may carry "vk": a `HyraxVk` over its document's rows, in place of "row_comms32".  Such instances are grouped by vk:
    ONE `HyraxVk.comm_lz` call per vk forms their comm_LZ, and the encodings it returns go into the transcript (no compress() call
    for them)."""
    curve = key.curve
    if not instances:
        return (True, []) if each else True
    right = len(instances[0]["point"]) - instances[0]["left"]
    n = 1 << right
    proofs, absorbed, bad = [], [], False
    by_vk, from_vk = {}, {}                                     # id(vk) -> (vk, [instance index]); instance index -> (comm_LZ, encoding)
    for i, it in enumerate(instances):
        vk = it.get("vk")
        if vk is None:
            continue
        if it.get("row_comms32") is not None:
            raise ValueError(f"instance {i}: \"vk\" stands in place of \"row_comms32\", not beside it")
        _check_vk(vk, curve, it["left"], "verify_eval_batch", i)
        by_vk.setdefault(id(vk), (vk, []))[1].append(i)
    for vk, idx in by_vk.values():
        jac, encs = vk.comm_lz([[x % p for x in instances[i]["point"][:vk.left]] for i in idx])
        for k, i in enumerate(idx):
            from_vk[i] = (jac[k], encs[k])
    for i, it in enumerate(instances):
        point, left, proof, challenge, q_of, q = it["point"], it["left"], it["proof"], it.get("challenge"), it.get("q_of"), it.get("q")
        h, blind_total = it.get("h"), it.get("blind_total")
        if len(point) - left != right:
            raise ValueError(f"instance {i}: 2^{len(point) - left} columns, the batch is over 2^{right}")
        if challenge is None and "rs" not in proof:
            raise ValueError("verify_eval_batch needs the round challenges: proof['rs'], or a challenge callable to draw them")
        if q is None and (challenge is None or q_of is None):
            raise ValueError("verify_eval_batch needs q, or a challenge callable and q_of to form it from the drawn r")
        if (h is None) != (blind_total is None):
            raise ValueError("h and blind_total come together or not at all")
        if i in from_vk:
            clz, cz = from_vk[i]
        else:
            clz = comm_lz(curve, it["row_comms32"], point[:left], p)
            cz = compress(key, clz)
        if challenge is not None:
            r_ipa = challenge("r", [cz, it["eval"]])
            if q_of is not None:
                q = q_of(r_ipa)
            rs = [challenge("challenge_r", [compress(key, L), compress(key, R)]) for L, R in zip(proof["L"], proof["R"])]
        else:
            rs = list(proof["rs"])
        if len(proof["L"]) != right or len(proof["R"]) != right or len(rs) != right:
            bad = True
            continue
        absorbed.append([cz, it["eval"] % p, proof["a_hat"]] + [compress(key, pt) for pair in zip(proof["L"], proof["R"]) for pt in pair])
        proofs.append({"comm": clz, "c": it["eval"] % p, "q": q, "L": proof["L"], "R": proof["R"], "rs": rs, "a_hat": proof["a_hat"],
                       "points": [list(point[left:])], "weights": [1], "h": h, "blind": None if blind_total is None else blind_total % p})
    if bad:                                                     # a proof of the wrong length verifies nowhere
        return (False, [False] * len(instances)) if each else False
    rho = [int(w) % p for w in weights(absorbed)]
    res = (check_fn or ipa_check_batch)(key, n, proofs, rho, each=each)
    return (res["accept"], res["each"]) if each else res["accept"]


# ---------------------------------------------------------------------------------------------------- 3k and the sum-check verifier
def matrix_evals(nifs: Nifs, num_cons_pad: int, num_vars_pad: int, r_x: Sequence[int], r_y: Sequence[int], *, is_mont: bool = False) -> List[int]:
    """reef_spartan_eval_matrices: [A~, B~, C~] at (r_x, r_y), len(r_x) = log2(num_cons_pad), len(r_y) = log2(2 num_vars_pad); ints in
    the form is_mont names.  The ctx needs its three matrices only."""
    def pow2(n):
        return n >= 2 and n & (n - 1) == 0
    if pow2(num_cons_pad) and pow2(num_vars_pad) and (len(r_x) != _rounds(num_cons_pad) or len(r_y) != _rounds(2 * num_vars_pad)):
        raise ValueError(f"pads ({num_cons_pad}, {num_vars_pad}) take {_rounds(num_cons_pad)} and {_rounds(2 * num_vars_pad)} point entries: "
                         f"r_x and r_y have {len(r_x)}, {len(r_y)}")
    xa, ya = (_arr(v) if len(v) else np.zeros((1, 4), np.uint64) for v in (r_x, r_y))   # illegal pads: the library says what is wrong
    out = np.zeros((3, 4), dtype=np.uint64)
    check(nifs._lib.reef_spartan_eval_matrices(nifs._h, num_cons_pad, num_vars_pad, xa.ctypes.data, ya.ctypes.data, bool(is_mont), out.ctypes.data))
    return _ints(out)


def matrix_evals_batch(nifs: Nifs, num_cons_pad: int, num_vars_pad: int, points: Sequence[Sequence[Sequence[int]]], *,
                       is_mont: bool = False) -> List[List[int]]:
    """reef_spartan_eval_matrices_batch (3o): [A~, B~, C~] at every (r_x, r_y) of `points` in one call -- one host wait, a matrix entry
    read once for two points.  Entry t is bit for bit `matrix_evals` at points[t].  An empty list makes no call."""
    m = len(points)
    if any(len(pt) != 2 for pt in points):
        raise ValueError("a point is a pair (r_x, r_y)")
    if m == 0:
        return []
    lx, ly = len(points[0][0]), len(points[0][1])
    for t, (r_x, r_y) in enumerate(points):
        if len(r_x) != lx or len(r_y) != ly:
            raise ValueError(f"point {t} has {len(r_x)} and {len(r_y)} entries, point 0 has {lx} and {ly}")

    def pow2(n):
        return n >= 2 and n & (n - 1) == 0
    if pow2(num_cons_pad) and pow2(num_vars_pad) and (lx != _rounds(num_cons_pad) or ly != _rounds(2 * num_vars_pad)):
        raise ValueError(f"pads ({num_cons_pad}, {num_vars_pad}) take {_rounds(num_cons_pad)} and {_rounds(2 * num_vars_pad)} point entries: "
                         f"r_x and r_y have {lx}, {ly}")
    xa = _arr([x for r_x, _ in points for x in r_x]) if lx else np.zeros((1, 4), np.uint64)   # illegal pads: the library says what is wrong
    ya = _arr([y for _, r_y in points for y in r_y]) if ly else np.zeros((1, 4), np.uint64)
    out = np.zeros((3 * m, 4), dtype=np.uint64)
    check(nifs._lib.reef_spartan_eval_matrices_batch(nifs._h, num_cons_pad, num_vars_pad, xa.ctypes.data, ya.ctypes.data, m, bool(is_mont),
                                                     out.ctypes.data))
    flat = _ints(out)
    return [flat[3 * t:3 * t + 3] for t in range(m)]


def _interp(ys: Sequence[int], r: int, p: int) -> int:
    """the polynomial through (0, ys[0]), (1, ys[1]), ... at r"""
    out = 0
    for i, y in enumerate(ys):
        num = den = 1
        for j in range(len(ys)):
            if j != i:
                num = num * (r - j) % p
                den = den * (i - j) % p
        out = (out + y * num * pow(den, -1, p)) % p
    return out


def _eq_entry(point: Sequence[int], i: int, p: int) -> int:
    """eq(point)[i], point[0] pairing with the most significant bit"""
    out, ell = 1, len(point)
    for j, t in enumerate(point):
        out = out * (t if (i >> (ell - 1 - j)) & 1 else 1 - t) % p
    return out


def _sumchecks_host(num_cons_pad, num_vars_pad, u, X, proof, challenge, p):
    """The host part of `_sumchecks`, up to the matrix evaluations: (ok, r_x, r_y, what `_sumchecks_final` needs)."""
    ell_x, ell_y = _rounds(num_cons_pad), _rounds(2 * num_vars_pad)
    outer, inner, co, ci = proof["outer"], proof["inner"], list(proof["claims_outer"]), list(proof["claims_inner"])
    if len(outer) != ell_x or len(inner) != ell_y or len(co) != 4 or len(ci) != 3 or 1 + len(X) > num_vars_pad:
        return False, [], [], None
    if any(len(ev) != 3 for ev in outer) or any(len(ev) != 2 for ev in inner):
        return False, [], [], None
    tau = [challenge("t", []) for _ in range(ell_x)]
    claim, r_x = 0, []
    for e0, e2, e3 in outer:
        r_x.append(challenge("outer", [e0, e2, e3]))
        claim = _interp([e0, (claim - e0) % p, e2, e3], r_x[-1], p)
    az, bz, cz, ex = co
    eq_tau = 1
    for a, b in zip(tau, r_x):
        eq_tau = eq_tau * (a * b + (1 - a) * (1 - b)) % p
    ok = claim == eq_tau * (az * bz - u * cz - ex) % p
    r = challenge("r", co)
    claim, r_y = (az + r * bz + r * r * cz) % p, []
    for e0, e2 in inner:
        r_y.append(challenge("inner", [e0, e2]))
        claim = _interp([e0, (claim - e0) % p, e2], r_y[-1], p)
    for name, drawn in (("tau", tau), ("r_x", r_x), ("r", r), ("r_y", r_y)):         # a transcript that records its challenges must agree
        ok = ok and (name not in proof or proof[name] == drawn)
    if not ok:
        return False, r_x, r_y, None
    eval_w = ci[2] % p
    eval_x = sum(_eq_entry(r_y[1:], j, p) * v for j, v in enumerate([u] + list(X))) % p
    z_ry = ((1 - r_y[0]) * eval_w + r_y[0] * eval_x) % p
    return True, r_x, r_y, (claim, r, z_ry, ci)


def _sumchecks_final(rest, evals: Sequence[int], p: int) -> bool:
    """The final comparisons of `_sumchecks` on [A~, B~, C~] at the proof's (r_x, r_y)."""
    claim, r, z_ry, ci = rest
    ea, eb, ec = evals
    abc = (ea + r * eb + r * r * ec) % p
    return claim == abc * z_ry % p and ci[0] == abc and ci[1] == z_ry


def _sumchecks(nifs, num_cons_pad, num_vars_pad, u, X, proof, challenge, p, evals_fn):
    ok, r_x, r_y, rest = _sumchecks_host(num_cons_pad, num_vars_pad, u, X, proof, challenge, p)
    if not ok:
        return False, r_x, r_y
    return _sumchecks_final(rest, (evals_fn or matrix_evals)(nifs, num_cons_pad, num_vars_pad, r_x, r_y), p), r_x, r_y


def verify_sumchecks(nifs: Optional[Nifs], num_cons_pad: int, num_vars_pad: int, u: int, X: Sequence[int], proof: dict,
                     challenge: Callable[[str, List[Any]], int], p: int, *, evals_fn=None) -> bool:
    """The verifier of 3g's transcript for an instance of which only u and X are known.  proof: {"outer", "claims_outer", "inner",
    "claims_inner"} as `spartan.prove` returns them (its "tau", "r_x", "r", "r_y", where present, must equal the re-drawn ones).
    Challenges in the prover's order: "t" x log2(num_cons_pad), "outer" per round, "r" after claims_outer, "inner" per round.  On the
    host: the round sums chained with e1 = claim - e0, claim_outer == eq(tau, r_x) (az bz - u cz - ex) with claims_outer as claimed
    (the opening proves eval_E; az, bz, cz are bound by the inner sum-check), eval_X = sum_j eq(r_y[1..])[j] (u || X)[j] and
    z(r_y) = (1 - r_y[0]) eval_W + r_y[0] eval_X.  On the device: `matrix_evals` on nifs (its matrices; no witness).  Then
    claim_inner == (A~ + r B~ + r^2 C~) z(r_y), claims_inner[0] against the same combination and claims_inner[1] against z(r_y).
    evals_fn(nifs, num_cons_pad, num_vars_pad, r_x, r_y) stands in for the device call (tests).  Canonical ints; False, never an
    exception, for a transcript that does not verify."""
    return _sumchecks(nifs, num_cons_pad, num_vars_pad, u % p, [x % p for x in X], proof, challenge, p, evals_fn)[0]


def verify_sumchecks_batch(nifs: Optional[Nifs], num_cons_pad: int, num_vars_pad: int, instances: Sequence[dict], p: int, *,
                           evals_fn=None) -> List[bool]:
    """`verify_sumchecks` for many proofs over one shape: a bool per instance.  instances: dicts with "u", "X", "proof" and "challenge"
    (each proof's own transcript).  The host part runs per proof; ONE `matrix_evals_batch` call then covers the proofs whose host
    checks passed (none is made when none passed), and the final comparisons run per proof.
    evals_fn(nifs, num_cons_pad, num_vars_pad, points) stands in for the device call (tests)."""
    out, live, points = [False] * len(instances), [], []
    for i, it in enumerate(instances):
        ok, r_x, r_y, rest = _sumchecks_host(num_cons_pad, num_vars_pad, it["u"] % p, [x % p for x in it["X"]], it["proof"], it["challenge"], p)
        if ok:
            live.append((i, rest))
            points.append((r_x, r_y))
    if live:
        evals = (evals_fn or matrix_evals_batch)(nifs, num_cons_pad, num_vars_pad, points)
        for (i, rest), ev in zip(live, evals):
            out[i] = _sumchecks_final(rest, ev, p)
    return out


def verify_snark(nifs: Optional[Nifs], key: MsmContext, gens_s, comm_e, comm_w, num_cons_pad: int, num_vars_pad: int, u: int, X: Sequence[int],
                 proof: dict, challenge: Callable[[str, List[Any]], int], p: int, *, evals_fn=None, check_fn=None) -> bool:
    """RelaxedR1CSSNARK::verify [R] on the device calls: `verify_sumchecks`, then `verify_opening` of [E, W] at (r_x, r_y[1..]) with
    eval_E = claims_outer[3] and eval_W = claims_inner[2], on one `challenge` in the prover's order.  proof: what
    `spartan.prove_with_opening` returns (the cross term as "cross_term" or "cross")."""
    ok, r_x, r_y = _sumchecks(nifs, num_cons_pad, num_vars_pad, u % p, [x % p for x in X], proof, challenge, p, evals_fn)
    if not ok:
        return False
    opening = {"cross": proof["cross"] if "cross" in proof else proof["cross_term"], "L": proof["L"], "R": proof["R"], "a_hat": proof["a_hat"]}
    return verify_opening(key, gens_s, comm_e, r_x, proof["claims_outer"][3], comm_w, r_y, proof["claims_inner"][2], opening, challenge, p,
                          check_fn=check_fn)
