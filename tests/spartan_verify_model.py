"""What the tests of the verifier's matrix evaluations (include/reef_msm.h 3k) share: the big-integer model of A~, B~, C~ at a point,
0/1 points that select one matrix position, a 257-row shape of arbitrary triples whose rows straddle every cut of the row pass, the
tamperings of a sum-check transcript, and cached shapes, instances and reference proves.  Nothing here is collected as a test."""
import functools
import random

import numpy as np

from gpu_drivers import spartan_shape
from oracle import pasta_ref
from oracle.ipa_oracle import affine, compress, msm
from oracle.r1cs_oracle import coef_pool, field, relaxed_instance
from oracle.spartan_oracle import Challenger, eq_evals, prove_ref, renumber

LONG_ROW, SEG = 128, 1024            # NIFS_LONG_ROW, NIFS_SEG of nifs_kernels.inc


# ---------------------------------------------------------------------------------------------------------------- the model
def model_evals(shape, num_vars_pad: int, r_x, r_y) -> list:
    """[A~, B~, C~](r_x, r_y) = sum_entries val eq(r_x)[row] eq(r_y)[col'], col' = renumber(col); duplicates are summed by the sum"""
    p, nv = shape["p"], shape["num_vars"]
    erx, ery = eq_evals(r_x, p), eq_evals(r_y, p)
    return [sum(v * erx[r] * ery[renumber(c, nv, num_vars_pad)] for r, c, v in zip(*shape[m])) % p for m in "ABC"]


def model_fn(shape):
    """the model as verify_sumchecks' evals_fn"""
    return lambda nifs, ncp, nvp, r_x, r_y: model_evals(shape, nvp, r_x, r_y)


def combine(evals, r: int, p: int) -> int:
    return (evals[0] + r * evals[1] + r * r * evals[2]) % p


def bits(i: int, ell: int) -> list:
    """the 0/1 point whose eq table is 1 at index i and 0 elsewhere (entry 0 = the most significant bit)"""
    return [(i >> (ell - 1 - j)) & 1 for j in range(ell)]


def entry_sums(shape, row: int, col: int) -> list:
    """the sum of the entries at (row, col) in A, B, C"""
    return [sum(v for r, c, v in zip(*shape[m]) if (r, c) == (row, col)) % shape["p"] for m in "ABC"]


def ells(pads):
    return pads[0].bit_length() - 1, (2 * pads[1]).bit_length() - 1


def random_point(pads, p: int, seed: int):
    rng = random.Random(seed)
    ell_x, ell_y = ells(pads)
    return [rng.randrange(p) for _ in range(ell_x)], [rng.randrange(p) for _ in range(ell_y)]


def forms(p: int, is_mont: bool):
    R = (1 << 256) % p
    return ((lambda v: v * R % p), (lambda v: v * pow(R, -1, p) % p)) if is_mont else ((lambda v: v), (lambda v: v))


# ---------------------------------------------------------------------------------------------------------------- shapes
@functools.lru_cache(maxsize=None)
def named_shape(curve: int, name: str):
    return spartan_shape(curve, name)


@functools.lru_cache(maxsize=None)
def named_instance(curve: int, name: str):
    return relaxed_instance(named_shape(curve, name)[0], 1, 11 + curve)


@functools.lru_cache(maxsize=None)
def named_prove(curve: int, name: str, seed: int):
    shape, pads = named_shape(curve, name)
    return prove_ref(shape, named_instance(curve, name), pads[0], pads[1], Challenger(shape["p"], seed))


# rows of the straddle shape: entries in (A, B, C).  The long-row threshold is on the SUM of the three, the segment cut per matrix.
STRADDLE_ROWS = {0: (100, 28, 0), 1: (100, 28, 1), 2: (SEG, 3, 0), 3: (5, SEG + 1, 0), 4: (0, 7, 2500), 130: (43, 43, 43), 131: (43, 43, 42),
                 254: (2 * SEG + 1, 0, 0), 255: (64, 64, 1), 256: (40, 40, 40)}
STRADDLE_PADS = (512, 512)


@functools.lru_cache(maxsize=None)
def straddle_shape(curve: int, c_empty: bool) -> dict:
    """257 rows (one row in the second block of 256) x 300 columns of arbitrary triples with coef_pool's classes: rows of exactly 128
    and 129 entries over the three matrices together, of 1024 and 1025 entries in one matrix, one of 2500, several long rows at
    once, the last row short; c_empty: C has no entry (its share of a listed row goes to A, so the totals stay)."""
    p = field(curve)
    rng = random.Random(900 + curve + 10 * c_empty)
    pool = coef_pool(p, rng)
    num_cons, num_vars, num_io = 257, 290, 9
    nz = num_vars + 1 + num_io
    mats = {m: ([], [], []) for m in "ABC"}
    for i in range(num_cons):
        counts = STRADDLE_ROWS.get(i) or tuple(0 if i % 11 == 5 else rng.randint(0, 6) for _ in range(3))
        if c_empty:
            counts = (counts[0] + counts[2], counts[1], 0)
        for m, k in zip("ABC", counts):
            for _ in range(k):
                mats[m][0].append(i)
                mats[m][1].append(rng.randrange(nz))
                mats[m][2].append(pool[rng.randrange(len(pool))])
    shape = {"num_cons": num_cons, "num_vars": num_vars, "num_io": num_io, "p": p}
    for m in "ABC":
        order = list(range(len(mats[m][0])))
        rng.shuffle(order)
        shape[m] = tuple([x[e] for e in order] for x in mats[m])
    lens = {i: sum(shape[m][0].count(i) for m in "ABC") for i in STRADDLE_ROWS}
    assert lens[0] == LONG_ROW and lens[1] == LONG_ROW + 1 and lens[131] == LONG_ROW and lens[130] == LONG_ROW + 1 and lens[255] == LONG_ROW + 1
    assert (len(shape["C"][0]) == 0) == c_empty
    return shape


# ---------------------------------------------------------------------------------------------------------------- tamperings
def tamperings(pf: dict, u: int, X, p: int):
    """(what, proof, u, X) with one value off by one: a round value of each sum-check, every claim, u, one X"""
    def bump(key, i, j=None):
        q = dict(pf)
        q[key] = [list(x) if isinstance(x, list) else x for x in pf[key]]
        if j is None:
            q[key][i] = (q[key][i] + 1) % p
        else:
            q[key][i][j] = (q[key][i][j] + 1) % p
        return q
    out = [("outer round", bump("outer", len(pf["outer"]) // 2, 1), u, X), ("inner round", bump("inner", len(pf["inner"]) - 1, 0), u, X)]
    out += [(f"claims_outer[{k}]", bump("claims_outer", k), u, X) for k in range(4)]
    out += [(f"claims_inner[{k}]", bump("claims_inner", k), u, X) for k in range(3)]
    out.append(("u", pf, (u + 1) % p, X))
    if X:
        out.append(("X", pf, u, [(X[0] + 1) % p] + list(X[1:])))
    return out


def replayable(pf: dict) -> dict:
    """the transcript as a verifier receives it: no recorded challenges"""
    return {k: pf[k] for k in ("outer", "claims_outer", "inner", "claims_inner")}


# ---------------------------------------------------------------------------------------------------------------- point operations
def comm_ops(curve: int, comm_e, comm_w, gens_s):
    """the caller's point operations of prove_with_opening: comm_a(r) as absorbed (compressed), q_of(r) affine"""
    def comm_a(r):
        return compress(curve, msm(curve, np.stack([comm_e, comm_w]), [1, r]))

    def q_of(r):
        return affine(curve, pasta_ref.scalar_mul(curve, gens_s, r))
    return comm_a, q_of
