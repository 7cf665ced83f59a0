"""Big-integer prover and verifier of the batched IPA opening of the final SNARK (include/reef_msm.h 3h).
TEST INFRASTRUCTURE ONLY -- only tests/, tools/ and smoke() may import it.

Restated from 3h's definitions, not from source text: nova-snark's NIFSForInnerProduct and InnerProductArgument::prove [R]
(EE::prove_batch over two instances, open_ref) and EE::verify_batch [R] (verify_open), over the curve operations of
oracle/pasta_ref.  Field elements are Python integers; points are what oracle.pasta_ref takes and returns (affine (k, 8) or
Jacobian (k, 12) uint64 limbs).  msm hands its scalars to pasta_ref as an (n, 4) uint64 array: _to_arr is this module's private
copy of that two-line conversion (the library's own is reef_amd._fe._arr, which oracle/ does not import).

PARITY WITH THE RUST CRATES IS UNPINNED: nothing here was run against nova-snark.  The reference pins nothing
recalled but what 3h lists.  It is checked by algebra (tests/test_spartan_open_host.py): the verifier folds the two instances
itself, rebuilds P_hat = sum r_i^2 L_i + comm_a + c Q + sum r_i^-2 R_i and compares it with a_hat <s, G> + a_hat <s, b> Q -- and a
changed L, R, a_hat, cross term or batch order makes the check fail."""
import random

import numpy as np

from oracle import pasta_ref
from oracle.r1cs_oracle import field


def _to_arr(vals) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


# ---------------------------------------------------------------------------------------------------------------- curve helpers
def msm(curve: int, points, scalars) -> np.ndarray:
    """sum scalars[i] points[i]: points affine (k, 8) or Jacobian (k, 12), scalars canonical ints; Jacobian out"""
    pts = np.ascontiguousarray(points, dtype=np.uint64)
    if pts.shape[-1] == 12:
        pts = pasta_ref.to_affine(curve, pts)
    pts = np.ascontiguousarray(pts.reshape(-1, 8))
    if pts.shape[0] > 4096:                                       # the oracle's Pippenger where the naive sum would take minutes
        return pasta_ref.msm_pippenger(curve, pts, _to_arr(scalars), mont=False, threads=8)
    return pasta_ref.msm_naive(curve, pts, _to_arr(scalars), mont=False)


def affine(curve: int, jac) -> np.ndarray:
    return pasta_ref.to_affine(curve, np.ascontiguousarray(jac, dtype=np.uint64))[0]


def compress(curve: int, jac) -> bytes:
    return pasta_ref.compress(curve, np.ascontiguousarray(jac, dtype=np.uint64))


def pad(v, n: int) -> list:
    return list(v) + [0] * (n - len(v))


def dot(x, y, p: int) -> int:
    return sum(a * b for a, b in zip(x, y)) % p


# ---------------------------------------------------------------------------------------------------------------- reference
def open_ref(curve: int, gens, gens_s, inst1: dict, inst2: dict, challenge) -> dict:
    """EE::prove_batch over two instances {comm, a, b} [R]: NIFSForInnerProduct, then InnerProductArgument::prove.  gens: the
    n = max(len b1, len b2) generators of gens_v (affine), gens_s: one affine point.  Challenges in 3h's label order."""
    p = field(curve)
    n = max(len(inst1["b"]), len(inst2["b"]))
    assert len(gens) == n and n >= 2 and n & (n - 1) == 0
    a1, b1, a2, b2 = (pad(inst[k], n) for inst in (inst1, inst2) for k in ("a", "b"))
    cross = (dot(a1, b2, p) + dot(a2, b1, p)) % p
    r = challenge("r", [cross])
    a = [(x + r * y) % p for x, y in zip(a1, a2)]
    b = [(x + r * y) % p for x, y in zip(b1, b2)]
    c = (dot(a1, b1, p) + r * r * dot(a2, b2, p) + r * cross) % p
    assert c == dot(a, b, p)
    comm_a = msm(curve, np.stack([inst1["comm"], inst2["comm"]]), [1, r])
    r_ipa = challenge("r", [compress(curve, comm_a), c])
    q = affine(curve, pasta_ref.scalar_mul(curve, gens_s, r_ipa))
    G = np.ascontiguousarray(gens, dtype=np.uint64)
    Ls, Rs, rs, trace = [], [], [], []
    while len(a) > 1:
        h = len(a) // 2
        c_l, c_r = dot(a[:h], b[h:], p), dot(a[h:], b[:h], p)
        Ls.append(msm(curve, np.vstack([G[h:], q[None]]), a[:h] + [c_l]))
        Rs.append(msm(curve, np.vstack([G[:h], q[None]]), a[h:] + [c_r]))
        rs.append(challenge("challenge_r", [compress(curve, Ls[-1]), compress(curve, Rs[-1])]))
        ri = pow(rs[-1], -1, p)
        a = [(a[i] * rs[-1] + a[h + i] * ri) % p for i in range(h)]
        b = [(b[i] * ri + b[h + i] * rs[-1]) % p for i in range(h)]
        G = pasta_ref.fold(curve, G, ri, rs[-1])
        trace.append({"a": a, "b": b})
    return {"cross": cross, "r": r, "c": c, "comm_a": comm_a, "r_ipa": r_ipa, "q": q, "L": Ls, "R": Rs, "rs": rs, "a_hat": a[0],
            "b_hat": b[0], "trace": trace}


# ---------------------------------------------------------------------------------------------------------------- the verifier
def s_vector(rs, p: int) -> list:
    """s_j = prod_i (bit of round i in j ? r_i : r_i^-1), round 0 on the most significant bit: G_hat = <s, G>, b_hat = <s, b>"""
    s = [1]
    for r in rs:
        ri = pow(r, -1, p)
        s = [x for e in s for x in (e * ri % p, e * r % p)]
    return s


def verify_open(curve: int, gens, gens_s, comm1, b1, eval1, comm2, b2, eval2, pf: dict, challenge) -> None:
    """EE::verify_batch [R]: the instances {comm, b, c} of [E, W] and the proof {cross, L, R, a_hat}."""
    p = field(curve)
    n = max(len(b1), len(b2))
    b1, b2 = pad(b1, n), pad(b2, n)
    r = challenge("r", [pf["cross"]])
    b = [(x + r * y) % p for x, y in zip(b1, b2)]
    c = (eval1 + r * r * eval2 + r * pf["cross"]) % p
    comm_a = msm(curve, np.stack([comm1, comm2]), [1, r])
    r_ipa = challenge("r", [compress(curve, comm_a), c])
    Q = pasta_ref.scalar_mul(curve, gens_s, r_ipa)
    assert len(pf["L"]) == len(pf["R"]) == n.bit_length() - 1, "rounds"
    rs = [challenge("challenge_r", [compress(curve, L), compress(curve, R)]) for L, R in zip(pf["L"], pf["R"])]
    pts = [comm_a, Q] + list(pf["L"]) + list(pf["R"])
    ks = [1, c] + [x * x % p for x in rs] + [pow(x, -2, p) for x in rs]
    p_hat = msm(curve, np.stack(pts), ks)
    s = s_vector(rs, p)
    g_hat = msm(curve, gens, s)
    b_hat = dot(s, b, p)
    a_hat = pf["a_hat"]
    rhs = msm(curve, np.stack([g_hat, Q]), [a_hat, a_hat * b_hat % p])
    assert compress(curve, p_hat) == compress(curve, rhs), "P_hat != a_hat G_hat + a_hat b_hat Q"


# ---------------------------------------------------------------------------------------------------------------- instances
def gens_of(curve: int, n: int):
    return pasta_ref.gen_bases_ap(curve, 7, 3, n), pasta_ref.gen_bases_ap(curve, 100003, 1, 1)[0]


def random_instances(curve: int, n1: int, n2: int, gens, seed: int):
    """[E, W]-shaped: instance 1 of length n1, instance 2 of n2 (a shorter than b, as E is to eq(r_x)), committed over gens"""
    p = field(curve)
    rng = random.Random(seed)
    insts = []
    for m in (n1, n2):
        a = [rng.randrange(p) for _ in range(max(1, m - 1))]
        b = [rng.randrange(p) for _ in range(m)]
        insts.append({"a": a, "b": b, "comm": msm(curve, gens[:len(a)], a), "eval": dot(a, b, p)})
    return insts
