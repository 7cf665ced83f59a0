"""The Hyrax consistency arguments of many proofs in lock-step on the GPU (reef_amd.hyrax.HyraxBatch over include/reef_msm.h 3p) against
the big-integer reference of oracle/hyrax_oracle.py, one reference run per proof, each proof with its own point, q and Challenger
seed: eval and lz_blind, a after eval_begin, every round's L and R (compressed), a and b after the first two rounds and after the
last, a_hat and b_hat, of every proof, in every call.  Both curves and input forms, symbols and field elements, the three modes (no
blinds, row blinds, row blinds and the h term), m = 1, 2, 3, 5 (m = 1 also against the single-argument API on the same ctx), the three
key kinds, the independence of the proofs, restarts and a single argument and commits interleaved with a batch, the errors, and one
shape with several blocks per proof."""
import random

import numpy as np
import pytest

from gpu_drivers import hyrax_points, key_of_kind, row_comms
from oracle import pasta_ref
from oracle.hyrax_oracle import blind_total, hyrax_ref, jacobian, verify_hyrax
from oracle.ipa_oracle import compress, gens_of, msm
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import Challenger, eq_evals
from reef_amd._fe import _arr

pytestmark = pytest.mark.gpu

_SYM = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _doc(curve, eb, n, seed, is_mont=False):
    """(what the device takes, the entries as ints): symbols of eb bytes, or field elements (is_mont form)"""
    p = field(curve)
    if eb != 32:
        top = {1: 256, 2: 65536, 4: 1 << 32}[eb]
        z = np.random.default_rng(seed).integers(0, top, size=n, dtype=np.uint64).astype(_SYM[eb])
        return z, [int(v) for v in z]
    r = random.Random(seed)
    ints = [r.randrange(p) for _ in range(n)]
    return _arr([v * (1 << 256) % p for v in ints] if is_mont else ints), ints


def _qs(curve, m, seed=0):
    """one point q per proof (and the batch's h): multiples of the drivers' two points"""
    q0, h = hyrax_points(curve)
    return [pasta_ref.to_affine(curve, pasta_ref.scalar_mul(curve, q0, 3 + 2 * i + 17 * seed))[0] for i in range(m)], h


class OneAt:
    """A Challenger whose `at`-th challenge is 1 (a fold with r = r^-1 = 1)"""

    def __init__(self, p, seed, at):
        self.inner, self.at, self.n = Challenger(p, seed), at, 0

    def __call__(self, label, absorbed):
        self.n += 1
        r = self.inner(label, absorbed)
        return 1 if self.n == self.at else r


def _forms(curve, is_mont):
    p = field(curve)
    R = (1 << 256) % p
    Ri = pow(R, -1, p)
    return ((lambda v: v * R % p), (lambda v: v * Ri % p)) if is_mont else ((lambda v: v), (lambda v: v))


def batch_steps(hb, key, curve, points, qs, challengers, refs, *, is_mont=False, h=None, blinds=None, trace=True, out=None):
    """The batch call by call (a generator: one step per call), each proof's challenges drawn by its own challenger from its own L and R
    as the reference draws them; every output of every proof with a reference (refs[i] not None) is compared with it in every call.
    blinds: per proof, `right` pairs (bl, br).  out (a list): receives one transcript dict per proof."""
    m, right = len(points), hb.right
    to, frm = _forms(curve, is_mont)
    form = "Montgomery" if is_mont else "canonical"
    full = [i for i in range(m) if refs[i] is not None]
    ev, lb = hb.eval_begin(key, [[to(x) for x in pt] for pt in points], is_mont=is_mont)
    tr = [{"eval": frm(ev[i]), "lz_blind": frm(lb[i]), "L": [], "R": [], "rs": []} for i in range(m)]
    for i in full:
        assert (tr[i]["eval"], tr[i]["lz_blind"]) == (refs[i]["eval"], refs[i]["lz_blind"]), f"proof {i}: eval, lz_blind ({form})"
        if trace:
            assert [frm(v) for v in hb.read(i, 0, 1 << right, to_mont=is_mont)] == refs[i]["lz"], f"proof {i}: a = LZ ({form})"
    yield "eval_begin"
    bl = (lambda k: [to(x) for i in range(m) for x in blinds[i][k]]) if h is not None else (lambda k: None)

    def take(k, L, Rp):
        for i in range(m):
            tr[i]["L"].append(L[i].copy())
            tr[i]["R"].append(Rp[i].copy())
            cl, cr = compress(curve, L[i]), compress(curve, Rp[i])
            if refs[i] is not None:
                assert (cl, cr) == (compress(curve, refs[i]["L"][k]), compress(curve, refs[i]["R"][k])), f"proof {i}: L, R round {k} ({form})"
            tr[i]["rs"].append(challengers[i]("challenge_r", [cl, cr]))
            if refs[i] is not None:
                assert tr[i]["rs"][k] == refs[i]["rs"][k]
    take(0, *hb.ipa_begin(np.stack(qs), h, bl(0), is_mont=is_mont))
    yield "ipa_begin"
    for k in range(right - 1):
        L, Rp = hb.ipa_round([to(tr[i]["rs"][k]) for i in range(m)], bl(k + 1), is_mont=is_mont)
        take(k + 1, L, Rp)
        if trace and (k < 2 or k == right - 2):
            for i in full:
                t = refs[i]["trace"][k]
                assert [frm(v) for v in hb.read(i, 0, len(t["a"]), to_mont=is_mont)] == t["a"], f"proof {i}: a after round {k} ({form})"
                assert [frm(v) for v in hb.read(i, 1, len(t["b"]), to_mont=is_mont)] == t["b"], f"proof {i}: b after round {k} ({form})"
        yield "ipa_round"
    a_hat, b_hat = hb.finish([to(tr[i]["rs"][-1]) for i in range(m)], is_mont=is_mont)
    for i in range(m):
        tr[i]["a_hat"], tr[i]["b_hat"] = frm(a_hat[i]), frm(b_hat[i])
    for i in full:
        assert (tr[i]["a_hat"], tr[i]["b_hat"]) == (refs[i]["a_hat"], refs[i]["b_hat"]), f"proof {i}: a_hat, b_hat ({form})"
        if trace:
            assert [frm(v) for v in hb.read(i, 0, 1, to_mont=is_mont)] == [refs[i]["a_hat"]], f"proof {i}: a after the last fold ({form})"
            assert [frm(v) for v in hb.read(i, 1, 1, to_mont=is_mont)] == [refs[i]["b_hat"]], f"proof {i}: b after the last fold ({form})"
    if out is not None:
        out[:] = tr
    yield "finish"


def run_batch(*args, **kw):
    out = []
    for _ in batch_steps(*args, out=out, **kw):
        pass
    return out


def single_steps(hx, key, ref, curve, point, q, *, is_mont=False, h=None, blinds=None, out=None):
    """The single argument (3i) call by call against its reference; out (a dict) receives the raw outputs"""
    to, frm = _forms(curve, is_mont)
    ev, lb = hx.eval_begin(key, [to(x) for x in point], is_mont=is_mont)
    assert (frm(ev), frm(lb)) == (ref["eval"], ref["lz_blind"])
    got = {"eval": ev, "lz_blind": lb, "a0": hx.read(0, len(ref["lz"]), to_mont=is_mont), "L": [], "R": []}
    yield
    bl = (lambda k: [to(x) for x in blinds[k]]) if h is not None else (lambda k: None)
    L, Rp = hx.ipa_begin(q, h, bl(0), is_mont=is_mont)
    got["L"].append(compress(curve, L))
    got["R"].append(compress(curve, Rp))
    assert (got["L"][0], got["R"][0]) == (compress(curve, ref["L"][0]), compress(curve, ref["R"][0]))
    yield
    for k, r in enumerate(ref["rs"][:-1]):
        L, Rp = hx.ipa_round(to(r), bl(k + 1), is_mont=is_mont)
        got["L"].append(compress(curve, L))
        got["R"].append(compress(curve, Rp))
        assert (got["L"][-1], got["R"][-1]) == (compress(curve, ref["L"][k + 1]), compress(curve, ref["R"][k + 1])), f"single argument: L, R round {k + 1}"
        t = ref["trace"][k]
        assert [frm(v) for v in hx.read(0, len(t["a"]), to_mont=is_mont)] == t["a"], f"single argument: a after round {k}"
        assert [frm(v) for v in hx.read(1, len(t["b"]), to_mont=is_mont)] == t["b"], f"single argument: b after round {k}"
        yield
    got["a_hat"], got["b_hat"] = hx.finish(to(ref["rs"][-1]), is_mont=is_mont)
    assert (frm(got["a_hat"]), frm(got["b_hat"])) == (ref["a_hat"], ref["b_hat"])
    if out is not None:
        out.update(got)
    yield


def _inputs(curve, num_vars, left, m, seed, mode):
    """m points, their q, h, the row blinds (mode >= 1) and per-proof round blinds (mode 2)"""
    p = field(curve)
    right = num_vars - left
    rng = random.Random(seed)
    points = [[rng.randrange(p) for _ in range(num_vars)] for _ in range(m)]
    qs, h = _qs(curve, m, seed % 5)
    row_blinds = [rng.randrange(p) for _ in range(1 << left)] if mode else None
    blinds = [[(rng.randrange(p), rng.randrange(p) if (k + i) % 2 else 0) for k in range(right)] for i in range(m)] if mode == 2 else None
    return points, qs, h, row_blinds, blinds


def _refs(curve, gens, ints, num_vars, left, points, qs, seeds, row_blinds, h, blinds):
    p = field(curve)
    return [hyrax_ref(curve, gens, ints, num_vars, left, points[i], qs[i], seeds[i] if callable(seeds[i]) else Challenger(p, seeds[i]), p,
                      row_blinds=row_blinds, h=h if blinds else None, blinds=blinds[i] if blinds else None) for i in range(len(points))]


# (curve, num_vars, elem_bytes, m, mode): mode 0 no blinds, 1 row blinds, 2 row blinds and the h term
CORE = [(0, 2, 1, 1, 0), (0, 2, 32, 3, 2), (1, 2, 1, 2, 1), (1, 2, 32, 5, 0),
        (0, 5, 1, 5, 2), (0, 5, 2, 2, 0), (0, 5, 4, 3, 1), (0, 5, 32, 1, 1),
        (1, 5, 1, 3, 0), (1, 5, 2, 1, 2), (1, 5, 4, 5, 1), (1, 5, 32, 2, 2),
        (0, 10, 1, 3, 1), (0, 10, 32, 2, 2), (1, 10, 1, 1, 2), (1, 10, 32, 5, 0)]


@pytest.mark.parametrize("curve,num_vars,eb,m,mode", CORE)
def test_batch_bit_exact_against_the_reference(gpu_lib, curve, num_vars, eb, m, mode):
    """num_vars = 2 has right = 1 (no ipa_round call at all); ten variables give several blocks of eq entries per proof.  m = 1 is also
    compared with the single-argument API on the same ctx, output for output."""
    from reef_amd.hyrax import HyraxBatch, HyraxEval
    p = field(curve)
    left = num_vars // 2
    right = num_vars - left
    n = (1 << num_vars) - (num_vars % 3)
    gens, _ = gens_of(curve, 1 << right)
    points, qs, h, row_blinds, blinds = _inputs(curve, num_vars, left, m, 1000 * eb + 10 * num_vars + curve, mode)
    seeds = [50 + 3 * i for i in range(m)]
    hh = h if mode == 2 else None
    with key_of_kind(curve, gens, "pre") as key:
        for is_mont in (False, True):
            to, frm = _forms(curve, is_mont)
            z, ints = _doc(curve, eb, n, 7 * num_vars + eb, is_mont)
            refs = _refs(curve, gens, ints, num_vars, left, points, qs, seeds, row_blinds, h, blinds)
            rb = [to(v) for v in row_blinds] if row_blinds else None
            with HyraxEval(curve, z, num_vars, left, row_blinds=rb, is_mont=is_mont) as hx, HyraxBatch(hx, m) as hb:
                tr = run_batch(hb, key, curve, points, qs, [Challenger(p, s) for s in seeds], refs, is_mont=is_mont, h=hh, blinds=blinds)
                if m == 1:
                    one = {}
                    for _ in single_steps(hx, key, refs[0], curve, points[0], qs[0], is_mont=is_mont, h=hh, blinds=blinds[0] if blinds else None, out=one):
                        pass
                    assert (frm(one["eval"]), frm(one["lz_blind"]), frm(one["a_hat"]), frm(one["b_hat"])) == \
                        (tr[0]["eval"], tr[0]["lz_blind"], tr[0]["a_hat"], tr[0]["b_hat"])
                    assert one["L"] == [compress(curve, x) for x in tr[0]["L"]] and one["R"] == [compress(curve, x) for x in tr[0]["R"]]
                b0 = eq_evals(points[-1][left:], p)        # the last proof's device transcript through the reference verifier
                comm = msm(curve, gens, refs[-1]["lz"])
                if mode:
                    comm = msm(curve, np.stack([pasta_ref.to_affine(curve, comm)[0], h]), [1, refs[-1]["lz_blind"]])
                total = blind_total(refs[-1]["lz_blind"], blinds[-1] if blinds else [], tr[-1]["rs"], p)
                verify_hyrax(curve, gens, qs[-1], comm, tr[-1]["eval"], b0, tr[-1], p, h=h if mode else None, lz_blind_total=total)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("with_h", [False, True])
def test_key_kinds_give_the_same_batch(gpu_lib, curve, with_h):
    """The pre-shifted bucket key, byte tables and a plain key: the rows take each kind's route, the encodings are the same"""
    from reef_amd.hyrax import HyraxBatch, HyraxEval
    p = field(curve)
    num_vars, left, m = 13, 2, 3                         # 2^11 columns: the byte-table range
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    points, qs, h, _, blinds = _inputs(curve, num_vars, left, m, 40 + curve, 2 if with_h else 0)
    z, ints = _doc(curve, 1, 1 << num_vars, 3)
    seeds = [9, 10, 11]
    refs = _refs(curve, gens, ints, num_vars, left, points, qs, seeds, None, h, blinds)
    with HyraxEval(curve, z, num_vars, left) as hx, HyraxBatch(hx, m) as hb:
        for kind in ("pre", "tables", "plain"):
            with key_of_kind(curve, gens, kind) as key:
                run_batch(hb, key, curve, points, qs, [Challenger(p, s) for s in seeds], refs, h=h if with_h else None, blinds=blinds,
                          trace=kind == "pre")


def test_the_proofs_of_a_batch_are_independent(gpu_lib):
    """Two identical proofs give identical outputs; a point of zeros and ones; a challenge r = 1 in one round; the proofs permuted"""
    from reef_amd.hyrax import HyraxBatch, HyraxEval
    curve, num_vars, left, m = 0, 7, 3, 4
    p = field(curve)
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    points, qs, h, row_blinds, blinds = _inputs(curve, num_vars, left, m, 66, 2)
    points[1], qs[1], blinds[1] = points[0], qs[0], blinds[0]
    points[2] = [(0x2D >> j) & 1 for j in range(num_vars)]
    mk = [lambda: Challenger(p, 1), lambda: Challenger(p, 1), lambda: Challenger(p, 2), lambda: OneAt(p, 3, 2)]
    z, ints = _doc(curve, 1, (1 << num_vars) - 3, 66)
    refs = _refs(curve, gens, ints, num_vars, left, points, qs, [f() for f in mk], row_blinds, h, blinds)
    assert refs[3]["rs"][1] == 1 and refs[2]["eval"] == ints[int("".join(map(str, points[2])), 2)]
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left, row_blinds=row_blinds) as hx, HyraxBatch(hx, m) as hb:
        tr = run_batch(hb, key, curve, points, qs, [f() for f in mk], refs, h=h, blinds=blinds)
        for k in ("eval", "lz_blind", "a_hat", "b_hat", "rs"):
            assert tr[0][k] == tr[1][k]
        assert all(np.array_equal(x, y) for x, y in zip(tr[0]["L"] + tr[0]["R"], tr[1]["L"] + tr[1]["R"]))
        perm = [2, 0, 3, 1]
        pick = lambda xs: [xs[i] for i in perm]          # noqa: E731
        tp = run_batch(hb, key, curve, pick(points), pick(qs), [mk[i]() for i in perm], pick(refs), h=h, blinds=pick(blinds))
        for j, i in enumerate(perm):
            for k in ("eval", "lz_blind", "a_hat", "b_hat", "rs"):
                assert tp[j][k] == tr[i][k]
            assert [compress(curve, x) for x in tp[j]["L"] + tp[j]["R"]] == [compress(curve, x) for x in tr[i]["L"] + tr[i]["R"]]


def test_restart_and_coexistence_with_the_single_argument(gpu_lib):
    """eval_begin mid-argument with a smaller m, then with m = m_max; a single reef_hyrax_* argument begun before the batch advances one
    call between every two batch calls and ends bit-exact, again and again; reef_hyrax_commit between two batch rounds changes
    nothing of either"""
    from reef_amd.hyrax import HyraxBatch, HyraxEval
    curve, num_vars, left, m_max = 1, 8, 4, 4
    p = field(curve)
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    points, qs, h, row_blinds, blinds = _inputs(curve, num_vars, left, m_max, 81, 2)
    z, ints = _doc(curve, 2, 250, 81)
    seeds = [21, 22, 23, 24]
    refs = _refs(curve, gens, ints, num_vars, left, points, qs, seeds, row_blinds, h, blinds)
    rng = random.Random(82)
    spoint = [rng.randrange(p) for _ in range(num_vars)]
    sblinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(num_vars - left)]
    sref = hyrax_ref(curve, gens, ints, num_vars, left, spoint, qs[2], Challenger(p, 30), p, row_blinds=row_blinds, h=h, blinds=sblinds)
    want_rows = b"".join(compress(curve, jacobian(curve, c)) for c in row_comms(curve, gens, ints, num_vars, left, row_blinds, h))
    done = []

    def singles(hx, key):
        while True:
            yield from single_steps(hx, key, sref, curve, spoint, qs[2], h=h, blinds=sblinds)
            done.append(1)

    def sub(lo, hi):
        return dict(h=h, blinds=blinds[lo:hi]), points[lo:hi], qs[lo:hi], [Challenger(p, s) for s in seeds[lo:hi]], refs[lo:hi]
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left, row_blinds=row_blinds) as hx, HyraxBatch(hx, m_max) as hb:
        single = singles(hx, key)
        next(single)                                       # the single argument's eval_begin comes before the batch exists to the device
        kw, pts, q, chs, rf = sub(0, 3)
        first = batch_steps(hb, key, curve, pts, q, chs, rf, **kw)
        for _ in range(3):                                 # eval_begin, ipa_begin, one round of three proofs, then left behind
            next(first)
            next(single)
        calls = 0
        for lo, hi in ((2, 4), (0, 4)):                    # a smaller m mid-argument, then m = m_max
            kw, pts, q, chs, rf = sub(lo, hi)
            for step in batch_steps(hb, key, curve, pts, q, chs, rf, **kw):
                calls += 1
                if step == "ipa_round" and calls % 2:
                    assert hx.commit(key, h) == want_rows
                next(single)
        assert len(done) >= 2


def test_errors_leave_the_batch_usable(gpu_lib):
    from reef_amd._ffi import ReefError
    from reef_amd.hyrax import HyraxBatch, HyraxEval
    curve, num_vars, left, m = 0, 8, 4, 3
    p = field(curve)
    gens, _ = gens_of(curve, 16)
    points, qs, h, _, blinds = _inputs(curve, num_vars, left, m, 5, 2)
    z, ints = _doc(curve, 2, 200, 5)
    seeds = [1, 2, 3]
    refs = _refs(curve, gens, ints, num_vars, left, points, qs, seeds, None, h, blinds)
    plain = _refs(curve, gens, ints, num_vars, left, points, qs, seeds, None, None, None)
    flat = lambda k: [x for i in range(m) for x in blinds[i][k]]   # noqa: E731
    rs = lambda k: [refs[i]["rs"][k] for i in range(m)]            # noqa: E731
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left) as hx:
        with pytest.raises(ReefError, match="m_max = 4097 exceeds 4096"):
            HyraxBatch(hx, 4097)
        with HyraxEval(curve, z, 14, 1) as wide, pytest.raises(ReefError, match="4096 \\* 8192 exceeds 16777216 entries"):
            HyraxBatch(wide, 4096)
        with HyraxBatch(hx, m) as hb:
            hb.m = m                                       # the front-end's own count of proofs, so that its length checks let the calls through
            for call in (lambda: hb.ipa_begin(np.stack(qs)), lambda: hb.ipa_round(rs(0)), lambda: hb.finish(rs(0)), lambda: hb.read(0, 0, 1)):
                with pytest.raises(ReefError, match="reef_hyrax_batch_eval_begin"):
                    call()
            assert hb.eval_begin(key, []) == ([], [])      # m = 0: nothing happens, nothing is begun
            with pytest.raises(ReefError, match="reef_hyrax_batch_eval_begin"):
                hb.read(0, 0, 1)
            with pytest.raises(ReefError, match="m = 4 exceeds the batch's m_max = 3"):
                hb.eval_begin(key, points + points[:1])
            with key_of_kind(curve, gens[:8], "pre") as short, pytest.raises(ReefError, match="8 points.*exactly 2\\^\\(num_vars - left_vars\\) = 16"):
                hb.eval_begin(short, points)
            with key_of_kind(1, gens_of(1, 16)[0], "pre") as other, pytest.raises(ReefError, match="curve 1"):
                hb.eval_begin(other, points)
            with key_of_kind(curve, gens, "pre") as part:
                part.set_window_split(0, 2)
                with pytest.raises(ReefError, match="window split"):
                    hb.eval_begin(part, points)
            with pytest.raises(ReefError, match="points\\[1\\]\\[2\\] is not below the modulus"):
                hb.eval_begin(key, [points[0], points[1][:2] + [p] + points[1][3:], points[2]])
            hb.eval_begin(key, points)
            for call, nxt in ((lambda: hb.ipa_round(rs(0)), "ipa_begin"), (lambda: hb.finish(rs(0)), "ipa_begin")):
                with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_batch_" + nxt):
                    call()
            with pytest.raises(ReefError, match="h given without"):
                hb.ipa_begin(np.stack(qs), h, None)
            with pytest.raises(ReefError, match="blinds\\[3\\] is not below the modulus"):
                hb.ipa_begin(np.stack(qs), h, flat(0)[:3] + [p] + flat(0)[4:])
            hb.ipa_begin(np.stack(qs), h, flat(0))
            for call, nxt in ((lambda: hb.ipa_begin(np.stack(qs)), "ipa_round"), (lambda: hb.finish(rs(0)), "ipa_round")):
                with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_batch_" + nxt):
                    call()
            with pytest.raises(ReefError, match="r\\[1\\] is zero"):
                hb.ipa_round([rs(0)[0], 0, rs(0)[2]], flat(1))
            with pytest.raises(ReefError, match="r\\[2\\] is not below the modulus"):
                hb.ipa_round([rs(0)[0], rs(0)[1], p], flat(1))
            hb.ipa_round(rs(0), flat(1))
            hb.ipa_round(rs(1), flat(2))
            hb.ipa_round(rs(2), None)                      # NULL blinds: zeros this round
            for call in (lambda: hb.ipa_round(rs(3), flat(3)), lambda: hb.ipa_begin(np.stack(qs))):
                with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_batch_finish"):
                    call()
            with pytest.raises(ReefError, match="r\\[0\\] is zero"):
                hb.finish([0] + rs(2)[1:])
            with pytest.raises(ReefError, match="proof 3 asked, the batch holds 3"):
                hb.read(3, 0, 1)
            with pytest.raises(ReefError, match="3 entries asked, the vector has 2"):
                hb.read(0, 1, 3)
            a_hat, b_hat = hb.finish(rs(3))                # after all these errors the argument ends: a_hat, b_hat depend on the challenges alone
            assert (a_hat, b_hat) == ([r["a_hat"] for r in refs], [r["b_hat"] for r in refs])
            with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_batch_eval_begin"):
                hb.finish(rs(3))
            hb.eval_begin(key, points)
            hb.ipa_begin(np.stack(qs))                     # no h term this time
            with pytest.raises(ReefError, match="took no h term"):
                hb.ipa_round(rs(0), flat(1))
            run_batch(hb, key, curve, points, qs, [Challenger(p, s) for s in seeds], plain)
            run_batch(hb, key, curve, points, qs, [Challenger(p, s) for s in seeds], refs, h=h, blinds=blinds, is_mont=True)


def test_a_larger_shape(gpu_lib):
    """num_vars = 18 (right = 9), 1-byte symbols, m = 16 on a pre-shifted key: rows x columns exceeds one block's stride at a size that is
    no toy.  Three of the 16 proofs against the reference in full; the others' device transcripts through the reference verifier, with
    comm_LZ formed from the a the device holds after eval_begin."""
    from reef_amd.hyrax import HyraxBatch, HyraxEval
    curve, num_vars, m = 0, 18, 16
    p = field(curve)
    left = right = 9
    gens, _ = gens_of(curve, 1 << right)
    points, qs, h, _, blinds = _inputs(curve, num_vars, left, m, 18, 2)
    z, ints = _doc(curve, 1, (1 << num_vars) - 77, 18)
    seeds = [100 + i for i in range(m)]
    full = (0, 7, 15)
    some = _refs(curve, gens, ints, num_vars, left, [points[i] for i in full], [qs[i] for i in full], [seeds[i] for i in full], None, h,
                 [blinds[i] for i in full])
    refs = [some[full.index(i)] if i in full else None for i in range(m)]
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left) as hx, HyraxBatch(hx, m) as hb:
        steps = batch_steps(hb, key, curve, points, qs, [Challenger(p, s) for s in seeds], refs, h=h, blinds=blinds, out=(tr := []))
        next(steps)
        lzs = {i: hb.read(i, 0, 1 << right) for i in range(m) if i not in full}
        for _ in steps:
            pass
    for i, lz in lzs.items():
        total = blind_total(0, blinds[i], tr[i]["rs"], p)
        verify_hyrax(curve, gens, qs[i], msm(curve, gens, lz), tr[i]["eval"], eq_evals(points[i][left:], p), tr[i], p, h=h, lz_blind_total=total)
