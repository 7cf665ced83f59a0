"""Row N6 on the host: a big-integer reference of one NIFS step (nova-snark's NIFS::prove [R]: the cross term T, the folds of
W, E, u, X) and of is_sat_relaxed, checked against itself; the library's new symbols; the loud failure without a GPU.

The reference pins nothing recalled but the layout z = W || u || X and the (row, col, value) triples.  It is correct by algebra:
if (W1, E1, u1, X1) satisfies A z o B z = u C z + E and a fresh (W2, E2 = 0, u2 = 1, X2) satisfies A z o B z = C z, the fold
with any r satisfies the relation again -- which the tests below check on random instances, with tampering caught.

Fresh instances come from a "layered" generator: every constraint's output variable is a product of two linear combinations of
inputs, u, X and earlier outputs, so the witness is computed constraint by constraint.  Coefficients mix +-1, powers of two,
small values, the edges of the library's small class (2^16 - 1, 2^16 and their negatives) and full-width values."""
import random

import numpy as np
import pytest

from oracle.pasta_oracle import P, Q

MAG = 0xFFFF                        # the largest coefficient magnitude the device takes as a one-word product (nifs_kernels.inc)


def field(curve: int) -> int:
    return Q if curve == 0 else P   # scalars of Pallas are Fq, of Vesta Fp


def to_arr(vals) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def from_arr(a) -> list:
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def to_mont(vals, p: int) -> list:
    return [v * (1 << 256) % p for v in vals]


# ---------------------------------------------------------------------------------------------------------------- reference
def matvec(mat, z, n: int, p: int) -> list:
    """R1CSShape::multiply_vec [R]: sum of val * z[col] per row, duplicate (row, col) entries summed."""
    out = [0] * n
    for r, c, v in zip(*mat):
        out[r] += v * z[c]
    return [x % p for x in out]


def cross_term(shape, run, fresh, p: int) -> list:
    """T = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - CZ1 of the running (W1, E1, u1, X1) and the fresh (W2, X2) instance."""
    n = shape["num_cons"]
    z1 = run["W"] + [run["u"]] + run["X"]
    z2 = fresh["W"] + [1] + fresh["X"]
    a1, b1, c1 = (matvec(shape[m], z1, n, p) for m in "ABC")
    a2, b2, c2 = (matvec(shape[m], z2, n, p) for m in "ABC")
    u1 = run["u"]
    return [(a1[i] * b2[i] + a2[i] * b1[i] - u1 * c2[i] - c1[i]) % p for i in range(n)]


def fold(run, fresh, t, r: int, p: int) -> dict:
    return {"W": [(a + r * b) % p for a, b in zip(run["W"], fresh["W"])],
            "E": [(a + r * b) % p for a, b in zip(run["E"], t)],
            "u": (run["u"] + r) % p,
            "X": [(a + r * b) % p for a, b in zip(run["X"], fresh["X"])]}


def bad_rows(shape, inst, p: int) -> list:
    """is_sat_relaxed without the commitment check: the rows where A z o B z != u C z + E."""
    n = shape["num_cons"]
    z = inst["W"] + [inst["u"]] + inst["X"]
    a, b, c = (matvec(shape[m], z, n, p) for m in "ABC")
    return [i for i in range(n) if (a[i] * b[i] - inst["u"] * c[i] - inst["E"][i]) % p]


def running_from_fresh(fresh, num_cons: int) -> dict:
    return {"W": list(fresh["W"]), "E": [0] * num_cons, "u": 1, "X": list(fresh["X"])}


# ---------------------------------------------------------------------------------------------------------------- generator
def coef_pool(p: int, rng: random.Random) -> list:
    pool = [1, p - 1, 1, p - 1, 2, p - 2, MAG, p - MAG, MAG + 1, p - MAG - 1, 3, 7, 1000, p - 12345]
    pool += [1 << k for k in range(1, 16)] + [p - (1 << k) for k in range(1, 16)] + [1 << 16, 1 << 40, p - (1 << 200)]
    pool += [rng.randrange(2, MAG) for _ in range(8)] + [rng.randrange(p) for _ in range(8)]
    return pool


def layered_shape(curve: int, num_cons: int, *, num_inputs: int = 8, num_io: int = 2, extra_vars: int = 0, seed: int = 1,
                  max_terms: int = 3, empty_every: int = 0, long_row: int = 0, dup_every: int = 0, shuffle: bool = True) -> dict:
    """A satisfiable R1CS shape.  Variables: num_inputs free inputs, one output per non-empty constraint, extra_vars unused ones
    (num_vars != num_cons).  Constraint i (unless empty_every divides i + 1): (lin. comb.) * (lin. comb.) = c_i out_i + (lin. comb.)
    over u, X, the inputs and earlier outputs; constraint num_cons // 2 has an A row of long_row entries; every dup_every-th
    entry is repeated (duplicates are summed)."""
    p = field(curve)
    rng = random.Random(seed)
    pool = coef_pool(p, rng)
    nz_pool = [c for c in pool if c % p]
    inv = {c: pow(c, -1, p) for c in nz_pool}
    outputs = [None] * num_cons
    nout = sum(1 for i in range(num_cons) if not (empty_every and (i + 1) % empty_every == 0))
    num_vars = num_inputs + nout + extra_vars
    u_col = num_vars
    avail = list(range(num_inputs)) + [u_col] + [num_vars + 1 + j for j in range(num_io)]
    rows = {m: ([], [], []) for m in "ABC"}
    plan = []                   # per constraint: (A terms, B terms, C other terms, c, out) for the witness
    nxt = num_inputs
    for i in range(num_cons):
        if empty_every and (i + 1) % empty_every == 0:
            plan.append(None)
            continue
        terms = {}
        for m in "AB":
            k = long_row if (m == "A" and long_row and i == num_cons // 2) else rng.randint(1, max_terms)
            terms[m] = [(avail[rng.randrange(len(avail))], pool[rng.randrange(len(pool))]) for _ in range(k)]
        terms["C"] = [(avail[rng.randrange(len(avail))], pool[rng.randrange(len(pool))]) for _ in range(rng.randint(0, 1))]
        c = nz_pool[rng.randrange(len(nz_pool))]
        out = nxt
        nxt += 1
        outputs[i] = out
        for m in "ABC":
            for col, v in terms[m] + ([(out, c)] if m == "C" else []):
                rows[m][0].append(i)
                rows[m][1].append(col)
                rows[m][2].append(v)
        plan.append((terms["A"], terms["B"], terms["C"], inv[c], out))
        avail.append(out)
    shape = {"num_cons": num_cons, "num_vars": num_vars, "num_io": num_io, "num_inputs": num_inputs, "plan": plan, "p": p}
    for m in "ABC":
        r, col, v = rows[m]
        if dup_every:
            # split an entry's value in two: the same (row, col) twice, which only a summing reader gets right
            for e in range(0, len(r), dup_every):
                part = rng.randrange(p)
                r.append(r[e]); col.append(col[e]); v.append((v[e] - part) % p)
                v[e] = part
        order = list(range(len(r)))
        if shuffle:
            rng.shuffle(order)
        shape[m] = ([r[e] for e in order], [col[e] for e in order], [v[e] for e in order])
    return shape


def fresh_instance(shape, seed: int) -> dict:
    """A satisfying (W, X) of the shape with u = 1, E = 0: outputs evaluated constraint by constraint."""
    p, nv = shape["p"], shape["num_vars"]
    rng = random.Random(seed)
    x = [rng.randrange(p) for _ in range(shape["num_io"])]
    z = [rng.randrange(p) for _ in range(nv)] + [1] + x        # inputs and extra vars random; outputs overwritten below
    for step in shape["plan"]:
        if step is None:
            continue
        ta, tb, tc, cinv, out = step
        a = sum(v * z[col] for col, v in ta)
        b = sum(v * z[col] for col, v in tb)
        rest = sum(v * z[col] for col, v in tc)
        z[out] = (a * b - rest) * cinv % p
    return {"W": z[:nv], "X": x}


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("curve", [0, 1])
def test_fresh_instances_of_the_generator_satisfy_the_relation(curve):
    shape = layered_shape(curve, 300, extra_vars=5, empty_every=17, dup_every=7, long_row=200, seed=curve + 3)
    for s in range(3):
        inst = running_from_fresh(fresh_instance(shape, s), shape["num_cons"])
        assert bad_rows(shape, inst, shape["p"]) == []


@pytest.mark.parametrize("curve", [0, 1])
def test_folding_keeps_instances_satisfiable_and_tampering_is_caught(curve):
    shape = layered_shape(curve, 200, num_io=3, extra_vars=9, empty_every=11, dup_every=5, seed=curve + 10)
    p, n = shape["p"], shape["num_cons"]
    rng = random.Random(99 + curve)
    run = running_from_fresh(fresh_instance(shape, 0), n)
    for step in range(1, 9):
        fresh = fresh_instance(shape, step)
        t = cross_term(shape, run, fresh, p)
        run = fold(run, fresh, t, rng.randrange(p), p)
        assert bad_rows(shape, run, p) == [], f"step {step}"
    assert run["u"] != 1 and any(run["E"])                       # a really relaxed instance by now
    k = next(i for i in range(n) if shape["plan"][i] is not None)
    bad = dict(run, E=list(run["E"]))
    bad["E"][k] = (bad["E"][k] + 1) % p
    assert bad_rows(shape, bad, p) == [k]
    bad = dict(run, W=list(run["W"]))
    out = shape["plan"][k][4]
    bad["W"][out] = (bad["W"][out] + 1) % p                      # an output variable: its own constraint breaks
    assert k in bad_rows(shape, bad, p)
    # a wrong T breaks the fold
    fresh = fresh_instance(shape, 50)
    t = cross_term(shape, run, fresh, p)
    t[k] = (t[k] + 1) % p
    assert bad_rows(shape, fold(run, fresh, t, 5, p), p) == [k]


def test_empty_rows_and_zero_coefficients_are_trivially_satisfied():
    shape = layered_shape(0, 40, empty_every=2, seed=5)
    inst = running_from_fresh(fresh_instance(shape, 1), 40)
    assert bad_rows(shape, inst, shape["p"]) == []
    assert all(shape["plan"][i] is None for i in range(1, 40, 2))


def test_array_round_trip():
    vals = [0, 1, Q - 1, 1 << 200, 0x1234567890ABCDEF << 64]
    assert from_arr(to_arr(vals)) == vals


def test_library_exports_the_nifs_symbols():
    from reef_amd import _ffi
    lib = _ffi.load()
    for name in ("reef_nifs_create", "reef_nifs_destroy", "reef_nifs_set_matrix", "reef_nifs_set_running", "reef_nifs_commit_T",
                 "reef_nifs_fold", "reef_nifs_read", "reef_nifs_check_relaxed"):
        assert hasattr(lib, name), name
        assert name in _ffi.declared_symbols()
    assert lib.reef_abi_version() == 7


def test_nifs_create_fails_loudly_without_gpu():
    from reef_amd import _ffi
    from reef_amd.nifs import Nifs
    if _ffi.load().reef_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_ffi.ReefError) as e:
        Nifs("pallas", 16, 16, 1)
    assert e.value.status == 3           # REEF_ERR_NO_GPU: no silent CPU fallback
