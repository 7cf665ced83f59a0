"""Big-integer model of relaxed R1CS and of one NIFS step (row N6; include/reef_msm.h 3f).
TEST INFRASTRUCTURE ONLY -- only tests/, tools/ and smoke() may import it.

Restated from the definitions, not from source text: nova-snark's NIFS::prove [R] (the cross term T, the folds of W, E, u, X),
R1CSShape::multiply_vec [R] (matvec) and is_sat_relaxed [R] without its commitment check (bad_rows), over the layout
z = W || u || X and (row, col, value) triples that 3f lists.  Field elements are Python integers.

PARITY WITH THE RUST CRATES IS UNPINNED: nothing here was run against nova-snark.  The model is correct by algebra:
if (W1, E1, u1, X1) satisfies A z o B z = u C z + E and a fresh (W2, E2 = 0, u2 = 1, X2) satisfies A z o B z = C z, the fold with
any r satisfies the relation again -- which tests/test_nifs_host.py checks on random instances, with tampering caught.

Fresh instances come from a "layered" generator: every constraint's output variable is a product of two linear combinations of
inputs, u, X and earlier outputs, so the witness is computed constraint by constraint.  Coefficients mix +-1, powers of two,
small values, the edges of the library's small class (2^16 - 1, 2^16 and their negatives) and full-width values."""
import random

from oracle.pasta_oracle import P, Q

MAG = 0xFFFF                        # the largest coefficient magnitude the device takes as a one-word product (nifs_kernels.inc)


def field(curve: int) -> int:
    return Q if curve == 0 else P   # scalars of Pallas are Fq, of Vesta Fp


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


def relaxed_instance(shape, steps: int, seed: int) -> dict:
    """A running instance with u != 1 and E != 0 after `steps` reference folds"""
    p, n = shape["p"], shape["num_cons"]
    rng = random.Random(seed)
    run = running_from_fresh(fresh_instance(shape, seed), n)
    for k in range(steps):
        fresh = fresh_instance(shape, seed + 100 + k)
        run = fold(run, fresh, cross_term(shape, run, fresh, p), rng.randrange(p), p)
    return run
