"""Big-integer prover and verifier of the Hyrax consistency argument, prove_eval (include/reef_msm.h 3i).
TEST INFRASTRUCTURE ONLY -- only tests/, tools/ and smoke() may import it.

Restated from 3i's definitions, not from source text, over the curve operations of oracle/pasta_ref: the bound rows LZ = L^T Z,
eval = <LZ, R>, sum_i L_i blind_i, comm_LZ = sum_i L_i C_i, and the IPA rounds of 3h (oracle/ipa_oracle.py) with the optional
per-round blinding term bl h (on L) and br h (on R).  Field elements are Python integers; points are what oracle.pasta_ref takes
and returns.

PARITY WITH THE RUST CRATES IS UNPINNED: nothing here was run against Reef's or nova-snark's Hyrax code.  The
reference is checked by algebra and against oracle/mle_oracle.py for LZ and eval (tests/test_hyrax_eval_host.py): honest
transcripts with and without the per-round h blinds pass verify_hyrax, a changed L, R, a_hat or challenge fails it."""
import numpy as np

from oracle import pasta_ref
from oracle.ipa_oracle import compress, dot, msm, s_vector
from oracle.spartan_oracle import eq_evals


def bound_ref(z, num_vars: int, left: int, point, p: int):
    """(LZ, eval): z zero-padded to 2^num_vars, row-major 2^left x 2^(num_vars - left); point[0] the most significant bit"""
    rows, cols = 1 << left, 1 << (num_vars - left)
    zz = [int(v) % p for v in z] + [0] * ((1 << num_vars) - len(z))
    L, Rv = eq_evals(point[:left], p), eq_evals(point[left:], p)
    lz = [sum(L[i] * zz[i * cols + j] for i in range(rows)) % p for j in range(cols)]
    return lz, dot(lz, Rv, p)


def hyrax_ref(curve: int, gens, z, num_vars: int, left: int, point, q, challenge, p: int, *, row_blinds=None, h=None, blinds=None,
              row_comms=None, lz=None) -> dict:
    """The whole argument, what the device must return call by call: each round's challenge is challenge("challenge_r",
    [compress(L), compress(R)]) as reef_amd.hyrax.prove_eval draws it.  q, h: affine points; blinds: right pairs (bl, br) with h.
    lz: LZ when it is known already (documents too large for bound_ref; z is then not read)."""
    L = eq_evals(point[:left], p)
    b = eq_evals(point[left:], p)
    if lz is None:
        lz, ev = bound_ref(z, num_vars, left, point, p)
    else:
        ev = dot(lz, b, p)
    lz_blind = dot(L, row_blinds, p) if row_blinds is not None else 0
    comm_lz = msm(curve, row_comms, L) if row_comms is not None else None
    a = list(lz)
    G = np.ascontiguousarray(gens, dtype=np.uint64)
    Ls, Rs, rs, trace = [], [], [], []
    for k in range(num_vars - left):
        n2 = len(a) // 2
        c_l, c_r = dot(a[:n2], b[n2:], p), dot(a[n2:], b[:n2], p)
        hp = [np.asarray(h, dtype=np.uint64).reshape(1, 8)] if h is not None else []
        Ls.append(msm(curve, np.vstack([G[n2:], q[None]] + hp), a[:n2] + [c_l] + ([blinds[k][0]] if hp else [])))
        Rs.append(msm(curve, np.vstack([G[:n2], q[None]] + hp), a[n2:] + [c_r] + ([blinds[k][1]] if hp else [])))
        r = challenge("challenge_r", [compress(curve, Ls[-1]), compress(curve, Rs[-1])])
        rs.append(r)
        ri = pow(r, -1, p)
        a = [(a[i] * r + a[n2 + i] * ri) % p for i in range(n2)]
        b = [(b[i] * ri + b[n2 + i] * r) % p for i in range(n2)]
        G = pasta_ref.fold(curve, G, ri, r)
        trace.append({"a": a, "b": b})
    return {"lz": lz, "eval": ev, "lz_blind": lz_blind, "comm_lz": comm_lz, "L": Ls, "R": Rs, "rs": rs, "a_hat": a[0], "b_hat": b[0],
            "trace": trace}


def verify_hyrax(curve: int, gens, q, comm_lz, eval_: int, b0, pf: dict, p: int, *, h=None, lz_blind_total: int = 0) -> None:
    """The round structure: P_hat = comm_LZ + eval q + sum r_k^2 L_k + sum r_k^-2 R_k must equal a_hat <s, G> + a_hat <s, b> q
    (+ lz_blind_total h when the argument is blinded: the commitment's blind folded with the round blinds).  rs: pf["rs"]."""
    rs = pf["rs"]
    pts = [comm_lz, q] + list(pf["L"]) + list(pf["R"])
    ks = [1, eval_ % p] + [x * x % p for x in rs] + [pow(x, -2, p) for x in rs]
    p_hat = msm(curve, np.stack([jacobian(curve, x) for x in pts]), ks)
    s = s_vector(rs, p)
    g_hat = msm(curve, gens, s)
    b_hat = dot(s, b0, p)
    a_hat = pf["a_hat"]
    rhs_pts, rhs_ks = [g_hat, jacobian(curve, q)], [a_hat, a_hat * b_hat % p]
    if h is not None:
        rhs_pts.append(jacobian(curve, h))
        rhs_ks.append(lz_blind_total % p)
    rhs = msm(curve, np.stack(rhs_pts), rhs_ks)
    assert compress(curve, p_hat) == compress(curve, rhs), "P_hat != a_hat G_hat + a_hat b_hat q"


def blind_total(lz_blind: int, blinds, rs, p: int) -> int:
    """The blind of P_hat: the commitment's, plus r_k^2 bl_k + r_k^-2 br_k per round"""
    t = lz_blind
    for (bl, br), r in zip(blinds, rs):
        t += r * r * bl + pow(r, -2, p) * br
    return t % p


def jacobian(curve: int, pt) -> np.ndarray:
    """a point as Jacobian limbs (12), from affine (8) or Jacobian"""
    a = np.ascontiguousarray(pt, dtype=np.uint64).reshape(-1)
    return a if a.size == 12 else pasta_ref.scalar_mul(curve, a, 1).reshape(-1)
