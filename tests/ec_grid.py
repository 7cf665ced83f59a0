"""The operand grid of the group-law tests: points in every representation ec.h accepts, the exceptional cases of each
addition, the lane layouts of the wave-wide paths, and the check of a raw result against Python integers.  Shared by
tests/test_ec_grid_host.py (the REEF_BOUNDS host build of ec.h) and tests/test_gpu_ec_bounds.py (the same grid on the device).

Forms.  A field element is nine 29-bit limbs in internal form (value = v * 2^261 mod M, plus a multiple of M).  An XYZZ point
is 36 words (X, Y, ZZ, ZZZ); for an affine (x, y) and a scale l it is (x l^2, y l^3, l^2, l^3), each coordinate lifted by k*M
with k up to 7, 3, 1, 1 -- all that the loose bounds "X < 8, Y < 4, ZZ, ZZZ < 2" allow.  An affine operand is the first 18 of
36 words, x canonical and y or y + M.  A table entry is 16 words (x, y canonical, packed), the identity all zero.

Limbs.  "Normalised" limbs are l0 < 2^29 and l1..l7 <= 2^29 + 7.  A limb can sit above 2^29 - 1 only where the strict limb of
the same value is at most 7, which a random value has with probability 2^-26 per limb: so the spread forms here are DESIGNED.
ZZ is chosen first, as a value whose limbs 1..7 are all in 1..7, among those that are l^2 for some l; X likewise among those
for which X / ZZ is the abscissa of a point.  `spread` then moves one unit of each upper limb down, and limbs 1..7 of these
coordinates all lie in 2^29 .. 2^29 + 7.  Multiples of M have limbs 5..7 zero and spread without help."""
import functools
import os
import random
import re

from mont_grid import MASK, RP, mont, value
from oracle.pasta_oracle import CURVES, sqrt_mod

CID = {"pallas": 0, "vesta": 1}
LMAX = MASK + 8                       # largest normalised limb 1..7
KMAX = (7, 3, 1, 1)                   # largest lift of X, Y, ZZ, ZZZ
EDGE = 1e-4                           # residues this close to M are not lifted to the very top (the bias checks keep 1e-5 clear)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Result bounds (multiples of M) and which coordinates have exact 29-bit limbs: the comments of ec.h, routine by routine.
# A difference (fe_sub) is normalised, a product exact.
DBL_AFFINE = ((5.1, 3.3, 1.13, 1.04), (False, False, True, True))
DBL = ((5.2, 3.4, 1.03, 1.02), (False, False, True, True))
MADD = ((5.2, 1.4, 1.03, 1.02), (True, True, True, True))
ADD = ((5.1, 1.25, 1.01, 1.01), (False, True, True, True))
INVARIANT = (6.0, 3.6, 1.6, 1.6)      # xyzz_to_mem


def limbs(v):
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def spread(v):
    """Limbs of v with limb 0 strict and every limb 1..7 that can be pushed above 2^29 - 1 (at most 2^29 + 7) pushed there."""
    l = limbs(v)
    for i in range(1, 8):
        if l[i + 1] > 0 and l[i] + (1 << 29) <= LMAX:
            l[i] += 1 << 29
            l[i + 1] -= 1
    assert value(l) == v and l[0] <= MASK and all(0 <= x <= LMAX for x in l[1:8])
    return l


def is_normalised(l):
    return l[0] <= MASK and all(x <= LMAX for x in l[1:8])


def consts(name, which):
    """A nine-limb constant of field_consts.h."""
    hdr = open(os.path.join(ROOT, "reef_amd", "csrc", "field_consts.h")).read()
    blk = hdr[hdr.index("struct FC<%d>" % CID[name]):]
    return [int(w.strip().rstrip("u"), 16) for w in re.search(r"\b%s\[9\] = \{([^}]*)\}" % which, blk).group(1).split(",")]


def fe_norm(d):
    """field.h: fe_norm on 32-bit limbs."""
    return [d[0] & MASK] + [(d[i] & MASK) + (d[i - 1] >> 29) for i in range(1, 8)] + [d[8] + (d[7] >> 29)]


class Operand:
    """Raw words of one operand, the multiples of M that bound its coordinates, and the point it stands for (None = identity)."""

    def __init__(self, words, pt):
        self.words = list(words) + [0] * (36 - len(words))
        self.pt = pt

    def bounds(self, m):
        return [value(self.words[9 * i:9 * i + 9]) / m + 1e-6 for i in range(4)]


class Case:
    """One lane: operands a and b (b affine for the mixed addition), flags (bit 0 a_known_empty, bit 1 p_inf), the expected
    point and how to check the raw result: ('point', bounds, exact) or ('words', the 36 words it must equal)."""

    def __init__(self, kind, a, b, flags, want, how):
        self.kind, self.a, self.b, self.flags, self.want, self.how = kind, a, b, flags, want, how


class Grid:
    def __init__(self, name):
        self.name, self.cid = name, CID[name]
        self.C = CURVES[name]
        self.m = m = self.C.base
        self.rng = random.Random(0xEC00 + self.cid)
        self.rinv = pow(RP, -1, m)
        self.one = limbs(RP % m)
        self.bias2 = consts(name, "BIAS2")
        step = self.C.mul(0x51ED27, self.C.gen)
        self.points = [self.C.mul(0xA11CE + self.cid, self.C.gen)]
        for _ in range(63):
            self.points.append(self.C.add(self.points[-1], step))
        self.lams = [1, m - 1, 2, (m - 1) // 2] + [self.rng.randrange(3, m) for _ in range(3)]
        self.t = 0                                        # representation counter: every operand takes the next lifts and scale

    # ---- field elements
    def to_int(self, v):
        return v * RP % self.m

    def from_int(self, v):
        return v * self.rinv % self.m

    def lift(self, r, k):
        """r + k*M, one multiple lower where the result would touch the bound the routines' bias checks keep clear of."""
        if k > 0 and r > (1 - EDGE) * self.m:
            k -= 1
        return r + k * self.m

    def designed(self, top_max):
        """A value whose strict limbs 1..7 are in 1..7 (so that spread lifts them all to 2^29 .. 2^29 + 7), limb 8 < top_max."""
        return value([self.rng.randrange(1 << 29)] + [self.rng.randrange(1, 8) for _ in range(7)] + [self.rng.randrange(1, top_max)])

    # ---- points
    def xyzz(self, pt, lam=None, ks=None, spread_zz=False, spread_x=False):
        """pt (not the identity) at scale lam with lifts ks; with spread_zz the scale is chosen for ZZ's limbs (lam is ignored),
        with spread_x -- together with spread_zz only -- pt too (it is ignored), and the point is returned in .pt."""
        m, t = self.m, self.t
        self.t += 1
        if ks is None:
            ks = (t % 8, (t // 2) % 4, (t // 3) % 2, (t // 5) % 2)
        if lam is None:
            lam = self.lams[(t + t // 7) % len(self.lams)]
        if spread_zz:
            while True:
                vzz = self.designed(int(2 * (1 - EDGE) * (1 << 22)) - 1)
                lam = sqrt_mod(self.from_int(vzz), m)
                if lam:
                    break
            zz = spread(vzz)
        else:
            zz = limbs(self.lift(self.to_int(lam * lam), ks[2]))
        if spread_x:
            assert spread_zz
            l2i = pow(lam * lam, -1, m)
            while True:
                vx = self.designed(int(8 * (1 - EDGE) * (1 << 22)) - 1)
                x = self.from_int(vx) * l2i % m
                y = sqrt_mod(x * x * x + 5, m)
                if y:
                    break
            pt = (x, y if t % 2 else m - y)
            xl = spread(vx)
        else:
            xl = limbs(self.lift(self.to_int(pt[0] * lam * lam), ks[0]))
        yl = limbs(self.lift(self.to_int(pt[1] * pow(lam, 3, m)), ks[1]))
        zzz = limbs(self.lift(self.to_int(pow(lam, 3, m)), ks[3]))
        assert self.C.is_on_curve(pt)
        return Operand(xl + yl + zz + zzz, pt)

    def rep(self, pt):
        """The next representation of pt: one in four with designed ZZ limbs."""
        return self.xyzz(pt, spread_zz=self.t % 4 == 3)

    def rep_own(self):
        """The next representation with designed X and ZZ limbs, of a point of its own."""
        return self.xyzz(None, spread_zz=True, spread_x=True)

    def identity(self, form):
        """form 0: all zero; otherwise ZZ in {0, M} (strict or spread) with X, Y, ZZZ zero or arbitrary within the loose bounds."""
        m, r = self.m, self.rng
        if form == 0:
            return Operand([0] * 36, None)
        zz = [[0] * 9, limbs(m), spread(m)][form % 3]
        if form % 2:
            x, y, zzz = ([0] * 9,) * 3
        else:
            x, y, zzz = (limbs(r.randrange(int(b * (1 - EDGE) * m))) for b in (8, 4, 2))
        return Operand(list(x) + list(y) + zz + list(zzz), None)

    IDENTITY_FORMS = 7                                    # forms 0..6: literal; ZZ = M strict / spread / 0, each with zero or arbitrary X, Y, ZZZ

    def affine(self, pt, t=None):
        """x canonical; y canonical, y + M, or y + M in spread limbs where they exist.  The identity is (0, 0)."""
        if pt is None:
            return Operand([0] * 18, None)
        if t is None:
            t = self.t
            self.t += 1
        y = self.to_int(pt[1])
        yl = limbs(y) if t % 3 == 0 else (limbs if t % 3 == 1 else spread)(self.lift(y, 1))
        return Operand(limbs(self.to_int(pt[0])) + yl, pt)

    def table_entry(self, pt):
        """16 words: x, y in internal form, canonical, packed."""
        if pt is None:
            return [0] * 16
        return [(self.to_int(c) >> (32 * i)) & 0xFFFFFFFF for c in pt for i in range(8)]

    def record(self, pt):
        """The 32 words of ec.h's affine_limbs for a table entry, from its layout comment."""
        if pt is None:
            return [0] * 11 + [1] + [0] * 20
        x, y = limbs(self.to_int(pt[0])), limbs(self.to_int(pt[1]))
        ny = fe_norm([b - l for b, l in zip(self.bias2, y)])          # fe_neg<C, 2>: 0 + BIAS2 - y, normalised
        assert value(ny) == 2 * self.m - value(y)
        return x[:8] + [x[8], y[8], ny[8], 0] + y[:8] + ny[:8] + [0] * 4

    # ---- the check of a raw result
    def parts(self, w):
        return [[int(x) for x in w[9 * i:9 * i + 9]] for i in range(4)]

    def point_of(self, w):
        """36 raw words -> the affine point (None for ZZ = 0 mod M); ZZ^3 = ZZZ^2 as field elements."""
        m = self.m
        X, Y, ZZ, ZZZ = (value(p) for p in self.parts(w))
        if ZZ % m == 0:
            return None
        zz, zzz = self.from_int(ZZ), self.from_int(ZZZ)
        assert pow(zz, 3, m) == zzz * zzz % m, "ZZ^3 != ZZZ^2"
        return (self.from_int(X) * pow(zz, -1, m) % m, self.from_int(Y) * pow(zzz, -1, m) % m)

    def check_point(self, w, want, bounds, exact, what=None):
        for p, b, ex in zip(self.parts(w), bounds, exact):
            assert all(x <= MASK for x in p[:8]) if ex else is_normalised(p), (what, [hex(x) for x in p])
            assert value(p) * 1000 < round(b * 1000) * self.m, (what, value(p) / self.m, b)
        got = self.point_of(w)
        assert got == want, (what, got, want)

    def check(self, case, w, what=None):
        what = (what, case.kind)
        if case.how[0] == "words":
            assert [int(x) for x in w] == case.how[1], what
            assert self.point_of(w) == case.want, what
        else:
            self.check_point(w, case.want, case.how[1], case.how[2], what)

    def madd_multiple(self, case):
        """The multiple j of M that U2 - X1 + 8M takes in a P + P case of the mixed addition: fe_mul_sub is the Montgomery
        product plus the bias minus the subtrahend, an exact integer."""
        a, p = self.parts(case.a.words), self.parts(case.b.words)
        v = mont(value(p[0]) * value(a[2]), self.m) + 8 * self.m - value(a[0])
        assert v % self.m == 0
        return v // self.m


KINDS_ADD = ["generic", "double", "cancel", "a_inf", "b_inf", "both_inf"]
KINDS_MADD = KINDS_ADD + ["a_known_empty"]


def add_case(g, kind, i):
    """One lane of xyzz_add / xyzz_add_coop."""
    C, P = g.C, g.points
    p, q = P[i % 64], P[(5 * i + 7) % 64]
    if p == q:
        q = P[(5 * i + 8) % 64]
    if kind == "generic":
        a = g.rep_own() if i % 4 == 0 else g.rep(p)
        b = g.rep(q)
        return Case(kind, a, b, 0, C.add(a.pt, q), ("point",) + ADD)
    if kind == "double":                                  # Q = P in another representation
        a = g.rep_own() if i % 2 == 0 else g.rep(p)
        b = g.rep(a.pt)
        return Case(kind, a, b, 0, C.add(a.pt, a.pt), ("point",) + DBL)
    if kind == "cancel":
        a = g.rep_own() if i % 2 == 0 else g.rep(p)
        b = g.rep(C.neg(a.pt))
        return Case(kind, a, b, 0, None, ("point",) + ADD)
    forms = g.IDENTITY_FORMS
    if kind == "a_inf":
        a, b = g.identity(i % forms), g.rep(q)
        return Case(kind, a, b, 0, q, ("words", b.words))
    if kind == "b_inf":
        a, b = g.rep(p), g.identity(i % forms)
        return Case(kind, a, b, 0, p, ("words", a.words))
    a, b = g.identity(i % forms), g.identity((i // forms + 2 * i) % forms)
    return Case(kind, a, b, 0, None, ("words", a.words))  # the select on b_inf is the last one: a comes out


def madd_case(g, kind, i):
    """One lane of xyzz_madd_flags(a, a_known_empty, p, p_inf)."""
    C, P = g.C, g.points
    p, q = P[i % 64], P[(5 * i + 7) % 64]
    if p == q:
        q = P[(5 * i + 8) % 64]
    if kind == "generic":
        a = g.rep_own() if i % 4 == 0 else g.rep(p)
        return Case(kind, a, g.affine(q), 0, C.add(a.pt, q), ("point",) + MADD)
    if kind == "double":
        a = g.rep_own() if i % 5 == 4 else g.xyzz(p, ks=(i % 8, (i // 8) % 4, (i // 2) % 2, (i // 4) % 2), spread_zz=i % 16 == 9)
        return Case(kind, a, g.affine(a.pt), 0, C.add(a.pt, a.pt), ("point",) + DBL_AFFINE)
    if kind == "cancel":
        a = g.rep_own() if i % 2 == 0 else g.rep(p)
        return Case(kind, a, g.affine(C.neg(a.pt)), 0, None, ("point",) + MADD)
    forms = g.IDENTITY_FORMS
    if kind in ("a_inf", "a_known_empty"):                # O + P = (x, y, 1, 1) with the operand's own limbs
        a = g.identity(i % forms if kind == "a_inf" else 0)
        b = g.affine(q)
        return Case(kind, a, b, 1 if kind == "a_known_empty" else 0, q, ("words", b.words[:18] + g.one + g.one))
    if kind == "b_inf":
        a = g.rep(p)
        return Case(kind, a, g.affine(None), 2, p, ("words", a.words))
    a = g.identity(i % forms)
    return Case(kind, a, g.affine(None), 2 | (i & 1 if i % forms == 0 else 0), None, ("words", a.words))


class Entry:
    """One lane of the loop form: acc + (+/-) table[index]."""

    def __init__(self, kind, acc, empty, index, neg, want, how):
        self.kind, self.a, self.empty, self.index, self.neg, self.want, self.how = kind, acc, empty, index, neg, want, how


def entry_cases(g, per_kind):
    """-> (table points, [Entry]): the matrix of the mixed addition with the operand given as a table entry and a sign."""
    C = g.C
    table = [None] + g.points[:31]                        # entry 0 is the identity record
    out = []
    for kind in KINDS_MADD:
        for i in range(per_kind):
            neg = bool((i + i // 2) % 2)
            idx = 1 + (3 * i) % 31
            e = table[idx]
            p = C.neg(e) if neg else e                    # the operand the loop adds
            other = table[1 + (3 * i + 11) % 31]
            pw = limbs(g.to_int(p[0])) + (g.record(e)[20:28] + [g.record(e)[10]] if neg else limbs(g.to_int(p[1])))
            if kind == "generic":
                a = g.rep(other)
                out.append(Entry(kind, a, 0, idx, neg, C.add(other, p), ("point",) + MADD))
            elif kind == "double":
                a = g.xyzz(p, ks=(i % 8, (i // 8) % 4, (i // 2) % 2, (i // 4) % 2), spread_zz=i % 16 == 9)
                out.append(Entry(kind, a, 0, idx, neg, C.add(p, p), ("point",) + DBL_AFFINE))
            elif kind == "cancel":
                out.append(Entry(kind, g.rep(C.neg(p)), 0, idx, neg, None, ("point",) + MADD))
            elif kind in ("a_inf", "a_known_empty"):
                a = g.identity(i % g.IDENTITY_FORMS if kind == "a_inf" else 0)
                out.append(Entry(kind, a, int(kind == "a_known_empty"), idx, neg, p, ("words", pw + g.one + g.one)))
            elif kind == "b_inf":
                a = g.rep(other)
                out.append(Entry(kind, a, 0, 0, neg, other, ("words", a.words)))
            else:
                a = g.identity(i % g.IDENTITY_FORMS)
                out.append(Entry(kind, a, int(i % g.IDENTITY_FORMS == 0 and i & 1), 0, neg, None, ("words", a.words)))
    return table, out


@functools.lru_cache(maxsize=None)
def pools(name, op, per_kind=64):
    """Per kind, per_kind cases of `op` ('add' or 'madd') over the representation grid; built once and not changed."""
    g = Grid(name)
    make, kinds = (add_case, KINDS_ADD) if op == "add" else (madd_case, KINDS_MADD)
    return g, {kind: [make(g, kind, i) for i in range(per_kind)] for kind in kinds}


def doubling_operands(g, n):
    """Operands of xyzz_dbl over the representation grid, every identity form among them."""
    ops = [g.identity(f) for f in range(g.IDENTITY_FORMS)]
    while len(ops) < n:
        i = len(ops)
        ops.append(g.rep_own() if i % 3 == 0 else g.rep(g.points[i % 64]))
    return ops


def layouts(kinds):
    """Lane layouts of the wave-wide paths: (label, [kind per lane]).  A run of 64 lanes is one wave of a one-wave kernel and one
    workgroup of the four-wave ones.  `kinds` are the exceptional kinds, 'double' among them."""
    out = []
    for k in kinds:
        out.append(("all " + k, [k] * 64))
        for lane in (0, 17, 63):
            out.append(("one %s at %d" % (k, lane), ["generic"] * lane + [k] + ["generic"] * (63 - lane)))
    mix = ["double", "cancel", "a_inf", "generic"]
    out.append(("side by side", [mix[i % 4] for i in range(64)]))
    out.append(("one double, one identity operand", ["generic"] * 9 + ["double"] + ["generic"] * 30 + ["a_inf"] + ["generic"] * 23))
    for tail in (37, 1):                                  # exceptional lanes only in the ragged last block; lane n - 1 is a P + P lane
        out.append(("ragged %d" % tail, ["generic"] * 256 + [kinds[i % len(kinds)] for i in range(tail - 1)] + ["double"]))
    out.append(("n = 150", [(["generic"] * 3 + kinds)[(i * 7) % (3 + len(kinds))] for i in range(150)]))
    for k in ["generic"] + list(kinds):
        out.append(("n = 1, " + k, [k]))
    return out


def lanes_of(pool, layout):
    """The cases of a layout: lane i takes the next unused case of its kind (cyclically)."""
    seen = {}
    out = []
    for k in layout:
        out.append(pool[k][seen.get(k, 0) % len(pool[k])])
        seen[k] = seen.get(k, 0) + 1
    return out


def zero_test_inputs(name):
    """The direct grid of fe_is_zero: for every j < 64, j*M (true), j*M with one bit flipped in each of limbs 1..8 (false, with the
    low limb kept: the exact compare decides), j*M +/- 1 (false), each in strict and in spread limbs.  -> [(limbs, expected)]"""
    m = CURVES[name].base
    rng = random.Random(0x15 + CID[name])
    out = []
    for j in range(64):
        for form in (limbs, spread):
            base = form(j * m)
            out.append((base, True))
            for i in range(1, 9):
                l = list(base)
                l[i] ^= 1 << rng.randrange(3 if l[i] > MASK else 22 if i == 8 else 29)    # a limb above 2^29 - 1 stays at most 2^29 + 7
                assert is_normalised(l) and value(l) < 64 * m
                out.append((l, False))
            for d in (-1, 1):
                if j * m + d >= 0:
                    out.append((form(j * m + d), False))
    return out


# ------------------------------------------------------------------------------------------------------------ the checks ----
# Each takes a `dev`: the host build or the device build behind the same five calls, on lists of words and Operands:
#   dev.pred(cid, op, rows, bounds) -> [0 | 1]                dev.one_wave(cid, op, a, b, flags) -> n x 36 words
#   dev.entry(cid, table, pay, acc, empty) -> (through the loop form, through the packed form, records), n x 36, n x 36, entries x 32
#   dev.chain(cid, table, pay) -> chains x steps x 36         dev.convert(cid, op, operands) -> n x 36
# and, on the device alone, dev.coop(cid, op, a, b) -> n x 36.
PRED_ZERO, PRED_LITERAL_ZERO, PRED_XYZZ_INF, PRED_AFFINE_INF = range(4)
OP_DBL_AFFINE, OP_DBL, OP_ADD, OP_NEG, OP_AFFINE_NEG, OP_FROM_AFFINE, OP_MADD_FLAGS = range(7)
CONV_TO_JACOBIAN, CONV_FROM_JACOBIAN, CONV_TO_AFFINE, CONV_COMPRESS = range(4)
CHAIN_BOUNDS = ((5.2, 3.3, 1.13, 1.04), (False,) * 4)     # either branch of the mixed addition; the pass-through cases lie inside it


def zero_grid_is_complete(name):
    """The condition on the direct fe_is_zero grid: per j < 64 and per limb form, j*M itself, a flip in each of limbs 1..8 and
    j*M +/- 1 (j*M - 1 from j = 1 on)."""
    m = CURVES[name].base
    seen = {}
    for l, want in zero_test_inputs(name):
        v = value(l)
        j = (v + m // 2) // m
        form = "strict" if all(x <= MASK for x in l[:8]) else "spread"
        assert l[0] < 64 or not want
        if v == j * m:
            assert want
            seen.setdefault((j, form), set()).add("zero")
            if j == 0:
                seen.setdefault((j, "spread"), set()).add("zero")     # 0 has one form only
        elif abs(v - j * m) == 1:
            assert not want
            seen.setdefault((j, form), set()).add(v - j * m)
        else:
            assert not want and l[0] == j                             # the low limb is kept: only the exact compare can tell
            base = limbs(j * m) if form == "strict" else spread(j * m)
            diff = [i for i in range(9) if l[i] != base[i]]
            assert len(diff) == 1 and bin(l[diff[0]] ^ base[diff[0]]).count("1") == 1
            seen.setdefault((j, form), set()).add("limb %d" % diff[0])
    full = {"zero", 1} | {"limb %d" % i for i in range(1, 9)}
    for j in range(64):
        for form in ("strict", "spread"):
            got = seen.get((j, form), set())
            if j == 0 and form == "spread":
                continue                                              # nothing to borrow from
            assert got >= full | ({-1} if j else set()), (j, form, got)
    return True


def check_predicates(dev, name):
    g = Grid(name)
    m = g.m
    rows = zero_test_inputs(name)
    got = dev.pred(g.cid, PRED_ZERO, [l for l, _ in rows], [[value(l) / m + 1e-6] * 4 for l, _ in rows])
    for (l, want), r in zip(rows, got):
        assert bool(r) == want, ([hex(x) for x in l], want)
    lit = [[0] * 9, limbs(m), spread(m), [1] + [0] * 8, [0] * 8 + [1]] + [[0] * i + [1 << 28] + [0] * (8 - i) for i in range(9)]
    got = dev.pred(g.cid, PRED_LITERAL_ZERO, lit, [[value(l) / m + 1e-6] * 4 for l in lit])
    assert [bool(r) for r in got] == [not any(l) for l in lit]
    ops = doubling_operands(g, 40)
    got = dev.pred(g.cid, PRED_XYZZ_INF, [o.words for o in ops], [o.bounds(m) for o in ops])
    assert [bool(r) for r in got] == [o.pt is None for o in ops]
    aff = [g.affine(None), Operand(limbs(g.to_int(0)) + limbs(m), None), Operand(limbs(m) + [0] * 9, None)] + [g.affine(p) for p in g.points[:9]]
    want = [True, False, False] + [False] * 9             # (0, 0) literally: (0, M) and (M, 0) are not the identity's encoding
    got = dev.pred(g.cid, PRED_AFFINE_INF, [o.words[:18] for o in aff], [o.bounds(m) for o in aff])
    assert [bool(r) for r in got] == want


def run_cases(dev, g, op, cases, what=None):
    out = dev.one_wave(g.cid, op, [c.a for c in cases], [c.b for c in cases], [c.flags for c in cases])
    for i, (c, w) in enumerate(zip(cases, out)):
        g.check(c, w, (what, i))
    return out


def all_cases(pool):
    return [c for k in pool for c in pool[k]]


def check_doubling(dev, name):
    g = Grid(name)
    ops = doubling_operands(g, 150)
    zero = [Operand([0] * 36, None)] * len(ops)
    for o, w in zip(ops, dev.one_wave(g.cid, OP_DBL, ops, zero, [0] * len(ops))):
        g.check_point(w, g.C.add(o.pt, o.pt), *DBL, what="xyzz_dbl")          # an identity of any form stays one
    aff = [g.affine(p) for p in g.points for _ in range(3)]
    for o, w in zip(aff, dev.one_wave(g.cid, OP_DBL_AFFINE, zero[:1] * len(aff), aff, [0] * len(aff))):
        g.check_point(w, g.C.add(o.pt, o.pt), *DBL_AFFINE, what="xyzz_dbl_affine")
    # the small ones: negations (Y' = 4M - Y, y' = 2M - y as integers, the identity (0, 0) kept) and xyzz_from_affine
    for o, w in zip(ops, dev.one_wave(g.cid, OP_NEG, ops, zero, [0] * len(ops))):
        p, q = g.parts(o.words), g.parts(w)
        assert (q[0], q[2], q[3]) == (p[0], p[2], p[3]) and value(q[1]) == 4 * g.m - value(p[1]) and is_normalised(q[1])
        assert g.point_of(w) == g.C.neg(o.pt)
    aff.append(g.affine(None))
    neg = dev.one_wave(g.cid, OP_AFFINE_NEG, zero[:1] * len(aff), aff, [0] * len(aff))
    lifted = dev.one_wave(g.cid, OP_FROM_AFFINE, zero[:1] * len(aff), aff, [0] * len(aff))
    for o, w, z in zip(aff, neg, lifted):
        p, q = g.parts(o.words), g.parts(w)
        assert q[0] == p[0] and not any(q[2]) and not any(q[3])
        if o.pt is None:
            assert not any(int(x) for x in w) and not any(int(x) for x in z)
        else:
            assert value(q[1]) == 2 * g.m - value(p[1]) and is_normalised(q[1])
            assert [int(x) for x in z] == o.words[:18] + g.one + g.one


def check_additions(dev, name):
    """xyzz_add and xyzz_madd_flags over their case matrices; -> the multiples j*M that U2 - X1 + 8M took in the P + P cases."""
    g, pool = pools(name, "add")
    run_cases(dev, g, OP_ADD, all_cases(pool), "xyzz_add")
    g, pool = pools(name, "madd")
    run_cases(dev, g, OP_MADD_FLAGS, all_cases(pool), "xyzz_madd_flags")
    return {g.madd_multiple(c) for c in pool["double"]}


def check_entries(dev, name):
    """The loop form against the packed form, bit for bit, and the records word for word; -> the multiples as above."""
    g = Grid(name)
    table, cases = entry_cases(g, 32)
    pay = [c.index | (int(c.neg) << 31) for c in cases]
    by_limbs, by_packed, records = dev.entry(g.cid, [g.table_entry(p) for p in table], pay, [c.a for c in cases], [c.empty for c in cases])
    for p, r in zip(table, records):
        assert [int(x) for x in r] == g.record(p), p
    assert any(c.index == 0 for c in cases) and {c.neg for c in cases if c.index == 0} == {False, True}       # an identity record, both signs
    js = set()
    for i, (c, wl, wp) in enumerate(zip(cases, by_limbs, by_packed)):
        assert [int(x) for x in wl] == [int(x) for x in wp], (i, c.kind, c.neg)
        g.check(c, wl, ("loop form", i, c.neg))
        if c.kind == "double":
            e = table[c.index]
            px = limbs(g.to_int(e[0]))
            v = mont(value(px) * value(g.parts(c.a.words)[2]), g.m) + 8 * g.m - value(g.parts(c.a.words)[0])
            assert v % g.m == 0
            js.add(v // g.m)
    return js


def chain_plans(g):
    """-> (table points, [chain]): a chain is a list of (entry index, negative).  Entry 0 is the identity; entries 1..3 are G', 2G', 3G'
    so that a walk over them keeps meeting its own sum (P + P), its negative and the identity."""
    C, r = g.C, random.Random(0xC4A1 + g.cid)
    base = g.points[5]
    table = [None, base, C.add(base, base), C.add(C.add(base, base), base)] + g.points[10:22]
    n = 300
    walk, s = [], 0                                       # small multiples of one point and identity entries, drawn back towards zero
    for _ in range(n):
        e, neg = r.randrange(4), bool(r.randrange(2))
        if s and r.randrange(4):
            neg = s > 0
        walk.append((e, neg))
        s += -e if neg else e
    planted = [(1, False), (1, False),                    # P + P at Z = 1: the first entry lands as (x, y, 1, 1)
               (1, True), (1, True),                      # 2P - P = P off Z = 1, then P - P: the identity as ZZ = 0 mod M beside leftover X, Y, ZZZ
               (5, False), (6, False), (5, True),         # on that identity: P5, P5 + P6, then P6 alone with ZZ != 1 ...
               (6, False),                                # ... + P6: the doubling branch right after a cancellation
               (0, False), (0, True),                     # identity entries, either sign
               (7, True), (7, False),                     # an immediate cancellation of the last addend
               (6, True), (6, True),                      # 2 P6 - P6 - P6: the identity again, reached off Z = 1
               (8, True), (8, True)]                      # O + (-P8), then P + P with a negative entry at Z = 1
    mixed = planted + [(4 + r.randrange(12), bool(r.randrange(2))) for _ in range(n - len(planted))]
    cancel = [((1 + k // 2 % 15), bool(k % 2)) for k in range(n)]                           # + P - P + Q - Q ...: all-cancelling
    nested = []
    while len(nested) < n:                                                                  # + P + Q - P - Q: cancels every fourth step
        a, b = 4 + r.randrange(12), 4 + r.randrange(12)
        nested += [(a, False), (b, False), (a, True), (b, True)]
    return table, [walk, mixed, cancel, nested[:n]]


def check_chains(dev, name):
    """Every intermediate accumulator against the running sum and the result bounds; -> how often a step was P + P, P - P, on an
    identity accumulator, an identity entry."""
    g = Grid(name)
    C = g.C
    table, chains = chain_plans(g)
    out = dev.chain(g.cid, [g.table_entry(p) for p in table], [[i | (int(s) << 31) for i, s in ch] for ch in chains])
    seen = {"double": 0, "cancel": 0, "on identity": 0, "identity entry": 0}
    for ci, (ch, res) in enumerate(zip(chains, out)):
        acc = None
        for k, ((i, s), w) in enumerate(zip(ch, res)):
            p = C.neg(table[i]) if s else table[i]
            seen["double"] += acc is not None and p == acc
            seen["cancel"] += acc is not None and p == C.neg(acc)
            seen["on identity"] += acc is None and k > 0
            seen["identity entry"] += p is None
            acc = C.add(acc, p)
            g.check_point(w, acc, *CHAIN_BOUNDS, what=(ci, k))
    assert g.point_of(out[2][-1]) is None and g.point_of(out[3][-1]) is None
    assert min(seen.values()) >= 8, seen
    return seen


def check_conversions(dev, name):
    g = Grid(name)
    C, m = g.C, g.m
    ops = doubling_operands(g, 60)
    jac = dev.convert(g.cid, CONV_TO_JACOBIAN, ops)
    for o, w in zip(ops, jac):
        w = [int(x) for x in w]
        assert not any(w[24:])
        if o.pt is None:
            assert not any(w)                             # (0, 0, 0)
        else:
            x, y, z = (sum(w[8 * c + i] << (32 * i) for i in range(8)) for c in range(3))
            assert max(x, y, z) < m and C.to_affine((C.from_mont(x), C.from_mont(y), C.from_mont(z))) == o.pt
    back = dev.convert(g.cid, CONV_FROM_JACOBIAN, [Operand([int(x) for x in w], o.pt) for o, w in zip(ops, jac)])
    for o, w in zip(ops, back):
        g.check_point(w, o.pt, (1.01, 1.01, 1.01, 1.01), (True,) * 4, what="round trip")
    for o, w in zip(ops, dev.convert(g.cid, CONV_TO_AFFINE, ops)):
        w = [int(x) for x in w]
        assert not any(w[18:])
        if o.pt is None:
            assert not any(w)                             # (0, 0)
        else:
            for c in range(2):
                l = w[9 * c:9 * c + 9]
                assert all(x <= MASK for x in l[:8]) and value(l) * 100 < 107 * m and g.from_int(value(l)) == o.pt[c]
    aff = [g.affine(None)] + [g.affine(q, t) for p in g.points[:12] for q in (p, C.neg(p)) for t in range(3)]
    for o, w in zip(aff, dev.convert(g.cid, CONV_COMPRESS, aff)):
        assert bytes(b for x in w[:8] for b in int(x).to_bytes(4, "little")) == C.compress(o.pt), o.pt        # identity: 32 zero bytes
    assert {o.pt[1] & 1 for o in aff[1:]} == {0, 1}
