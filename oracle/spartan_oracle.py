"""Big-integer prover and verifier of the two sum-checks of the final SNARK (row N5; include/reef_msm.h 3g).
TEST INFRASTRUCTURE ONLY -- only tests/, tools/ and smoke() may import it.

Restated from 3g's definitions, not from source text: nova-snark's RelaxedR1CSSNARK::prove [R] -- the outer cubic sum-check over
eq(tau), AZ, BZ, u CZ + E and the inner quadratic one over ABC and the padded z -- with EqPolynomial::evals [R] (eq_evals) and
compute_eval_table_sparse [R] (abc_table).  The transcript is a seeded stand-in (Challenger), not nova's Keccak.  The R1CS model
is oracle/r1cs_oracle.py; field elements are Python integers.

PARITY WITH THE RUST CRATES IS UNPINNED: nothing here was run against nova-snark.  The reference pins nothing
recalled but what 3g lists.  It is checked by algebra (tests/test_spartan_host.py): every round's g(0) + g(1) equals the running
claim, the outer final claim equals eq(tau, r_x) (AZ BZ - u CZ - E) at r_x with every term evaluated straight from the unpadded
shape, and the inner one ABC(r_y) z(r_y) with ABC taken straight from the triples -- and a broken row makes the outer identity fail."""
import hashlib

from oracle.r1cs_oracle import matvec


# ---------------------------------------------------------------------------------------------------------------- reference
class Challenger:
    """A seeded stand-in for nova's Keccak transcript: each challenge hashes the seed, a counter, the label and what was absorbed."""

    def __init__(self, p: int, seed: int = 0):
        self.p, self.seed, self.n = p, seed, 0

    def __call__(self, label: str, absorbed) -> int:
        self.n += 1
        h = hashlib.sha256(f"{self.seed}/{self.n}/{label}/{','.join(map(str, absorbed))}".encode()).digest()
        return int.from_bytes(h + hashlib.sha256(h).digest(), "little") % self.p


def eq_evals(t, p: int) -> list:
    """eq(t)[i] = prod_j (bit_j(i) ? t_j : 1 - t_j), t_0 pairing with the most significant bit (EqPolynomial::evals [R])."""
    ev = [1]
    for tj in t:
        ev = [x for e in ev for x in (e * (1 - tj) % p, e * tj % p)]
    return ev


def eq_at(a, b, p: int) -> int:
    out = 1
    for x, y in zip(a, b):
        out = out * (x * y + (1 - x) * (1 - y)) % p
    return out


def bind_top(x, r: int, p: int) -> list:
    n = len(x) // 2
    return [(x[i] + r * (x[i + n] - x[i])) % p for i in range(n)]


def interp(ys, r: int, p: int) -> int:
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


def renumber(col: int, num_vars: int, num_vars_pad: int) -> int:
    return col if col < num_vars else col + num_vars_pad - num_vars


def check_pads(shape, num_cons_pad: int, num_vars_pad: int):
    def pow2(n):
        return 2 <= n <= 1 << 24 and n & (n - 1) == 0
    return (pow2(num_cons_pad) and pow2(num_vars_pad) and num_cons_pad >= shape["num_cons"] and num_vars_pad >= shape["num_vars"]
            and shape["num_io"] < num_vars_pad)


def padded_z(inst, num_vars_pad: int) -> list:
    """z = W || 0 || u || X || 0, 2 num_vars_pad entries"""
    w = inst["W"] + [0] * (num_vars_pad - len(inst["W"]))
    ux = [inst["u"]] + inst["X"]
    return w + ux + [0] * (num_vars_pad - len(ux))


def abc_table(shape, evals_rx, r: int, num_vars_pad: int, p: int) -> list:
    """compute_eval_table_sparse [R], combined: ABC[col'] = sum eq(r_x)[row] (A + r B + r^2 C)[row][col], renumbered columns"""
    out = [0] * (2 * num_vars_pad)
    for coef, m in ((1, "A"), (r, "B"), (r * r % p, "C")):
        for row, col, v in zip(*shape[m]):
            c = renumber(col, shape["num_vars"], num_vars_pad)
            out[c] = (out[c] + coef * evals_rx[row] * v) % p
    return out


def prove_ref(shape, inst, num_cons_pad: int, num_vars_pad: int, challenge, strict: bool = True) -> dict:
    """Both sum-checks as RelaxedR1CSSNARK::prove [R] runs them; asserts g(0) + g(1) = claim every round (strict: an instance
    that satisfies the relation, so that the outer sum is 0)."""
    assert check_pads(shape, num_cons_pad, num_vars_pad)
    p, n = shape["p"], shape["num_cons"]
    z = inst["W"] + [inst["u"]] + inst["X"]
    pad = [0] * (num_cons_pad - n)
    az, bz, cz = (matvec(shape[m], z, n, p) + pad for m in "ABC")
    e = list(inst["E"]) + pad
    d = [(inst["u"] * c + x) % p for c, x in zip(cz, e)]
    ell_x = num_cons_pad.bit_length() - 1
    ell_y = (2 * num_vars_pad).bit_length() - 1
    tau = [challenge("t", []) for _ in range(ell_x)]
    tabs = [eq_evals(tau, p), az, bz, d]
    claim, outer, r_x = 0, [], []
    for _ in range(ell_x):
        h = len(tabs[0]) // 2
        ev = []
        for t in range(4):
            s = 0
            for i in range(h):
                q, a, b, dd = ((x[i] + t * (x[i + h] - x[i])) % p for x in tabs)
                s += q * (a * b - dd)
            ev.append(s % p)
        assert not strict or (ev[0] + ev[1]) % p == claim
        outer.append([ev[0], ev[2], ev[3]])
        r_x.append(challenge("outer", outer[-1]))
        claim = interp(ev, r_x[-1], p)
        tabs = [bind_top(x, r_x[-1], p) for x in tabs]
    evals_rx = eq_evals(r_x, p)
    claims_outer = [tabs[1][0], tabs[2][0], sum(a * b for a, b in zip(evals_rx, cz)) % p, sum(a * b for a, b in zip(evals_rx, e)) % p]
    r = challenge("r", claims_outer)
    outer_final = claim
    claim = (claims_outer[0] + r * claims_outer[1] + r * r * claims_outer[2]) % p
    tabs = [abc_table(shape, evals_rx, r, num_vars_pad, p), padded_z(inst, num_vars_pad)]
    inner, r_y = [], []
    for _ in range(ell_y):
        h = len(tabs[0]) // 2
        a, b = tabs
        ev = [sum((a[i] + t * (a[i + h] - a[i])) * (b[i] + t * (b[i + h] - b[i])) for i in range(h)) % p for t in range(3)]
        assert not strict or (ev[0] + ev[1]) % p == claim
        inner.append([ev[0], ev[2]])
        r_y.append(challenge("inner", inner[-1]))
        claim = interp(ev, r_y[-1], p)
        tabs = [bind_top(x, r_y[-1], p) for x in tabs]
    w = inst["W"] + [0] * (num_vars_pad - shape["num_vars"])
    eval_w = sum(a * b for a, b in zip(eq_evals(r_y[1:], p), w)) % p
    return {"tau": tau, "outer": outer, "r_x": r_x, "claims_outer": claims_outer, "r": r, "inner": inner, "r_y": r_y,
            "claims_inner": [tabs[0][0], tabs[1][0], eval_w], "outer_final": outer_final, "inner_final": claim}


# ---------------------------------------------------------------------------------------------------------------- the verifier
def verify(shape, inst, num_cons_pad: int, num_vars_pad: int, pf: dict, challenge) -> None:
    """What the verifier checks, with every evaluation taken straight from the unpadded shape and instance (no padded table):
    challenges re-derived, round sums chained, and the two final claims."""
    p, n, nv = shape["p"], shape["num_cons"], shape["num_vars"]
    ell_x = num_cons_pad.bit_length() - 1
    tau = [challenge("t", []) for _ in range(ell_x)]
    assert tau == pf["tau"]
    claim, r_x = 0, []
    for ev in pf["outer"]:
        e0, e2, e3 = ev
        r_x.append(challenge("outer", ev))
        claim = interp([e0, (claim - e0) % p, e2, e3], r_x[-1], p)
    assert r_x == pf["r_x"]
    # AZ, BZ, CZ, E at r_x: eq(r_x) at each row index (rows >= num_cons are zero)
    z = inst["W"] + [inst["u"]] + inst["X"]
    erx = eq_evals(r_x, p)[:n]
    az, bz, cz = (sum(a * b for a, b in zip(erx, matvec(shape[m], z, n, p))) % p for m in "ABC")
    ex = sum(a * b for a, b in zip(erx, inst["E"])) % p
    assert pf["claims_outer"] == [az, bz, cz, ex]
    assert claim == eq_at(tau, r_x, p) * (az * bz - inst["u"] * cz - ex) % p, "outer final claim"
    r = challenge("r", pf["claims_outer"])
    claim, r_y = (az + r * bz + r * r * cz) % p, []
    for ev in pf["inner"]:
        e0, e2 = ev
        r_y.append(challenge("inner", ev))
        claim = interp([e0, (claim - e0) % p, e2], r_y[-1], p)
    assert r_y == pf["r_y"]
    ery = eq_evals(r_y, p)
    abc = 0
    for coef, m in ((1, "A"), (r, "B"), (r * r % p, "C")):
        for row, col, v in zip(*shape[m]):
            abc += coef * erx[row] * ery[renumber(col, nv, num_vars_pad)] * v
    abc %= p
    eq1 = eq_evals(r_y[1:], p)
    eval_w = sum(a * b for a, b in zip(eq1, inst["W"])) % p
    ux = sum(a * b for a, b in zip(eq1, [inst["u"]] + inst["X"])) % p
    zr = ((1 - r_y[0]) * eval_w + r_y[0] * ux) % p
    assert pf["claims_inner"] == [abc, zr, eval_w]
    assert claim == abc * zr % p, "inner final claim"


def next_pow2(n: int) -> int:
    return max(2, 1 << (n - 1).bit_length())
