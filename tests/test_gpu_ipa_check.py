"""The verifier's IPA check on the GPU (reef_amd.verify over include/reef_msm.h 3j) against the big-integer verifiers of
oracle/ipa_oracle.py and oracle/hyrax_oracle.py, bit-exact after compress: the intermediates P_hat, G_hat, b_hat on random inputs at
every size where the s kernel takes another path; honest transcripts of the reference provers and of the device provers accept;
every tamper rejects with REEF_OK (and makes the oracle verifier raise as well); the three key kinds; b built on the device against
b uploaded; the comparison kernel on identities and re-scaled points; the argument errors; one 2^15 case on the bucket pipeline."""
import functools
import random

import numpy as np
import pytest

from gpu_drivers import (hyrax_points, key_of_kind, open_shape, opening_instances, row_comms, set_running, upload_shape)
from oracle import pasta_ref
from oracle.hyrax_oracle import blind_total, hyrax_ref, verify_hyrax
from oracle.ipa_oracle import affine, compress, dot, gens_of, msm, open_ref, pad, random_instances, s_vector, verify_open
from oracle.r1cs_oracle import field, relaxed_instance
from oracle.spartan_oracle import Challenger, eq_evals

pytestmark = pytest.mark.gpu


def _forms(p, is_mont):
    R = (1 << 256) % p
    return ((lambda v: v * R % p), (lambda v: v * pow(R, -1, p) % p)) if is_mont else ((lambda v: v), (lambda v: v))


def _point(curve, seed):
    """a Jacobian point nobody knows a relation for"""
    return pasta_ref.scalar_mul(curve, pasta_ref.gen_bases_ap(curve, 900 + seed, 1, 1)[0], 0x1234567 + seed).reshape(12)


def _rescaled(curve, jac, lam):
    """the same point with Z scaled by lam: (lam^2 X, lam^3 Y, lam Z), coordinates in pasta Montgomery form over the base field"""
    from reef_amd._fe import _arr, _ints
    pb = field(1 - curve)                                  # the curve's base field is the other curve's scalar field
    Rinv = pow((1 << 256) % pb, -1, pb)
    x, y, z = _ints(np.asarray(jac, dtype=np.uint64).reshape(3, 4))
    lm = lam * (1 << 256) % pb
    mul = lambda a, b: a * b * Rinv % pb                   # Montgomery product
    l2 = mul(lm, lm)
    return _arr([mul(x, l2), mul(y, mul(l2, lm)), mul(z, lm)]).reshape(12)


@functools.lru_cache(maxsize=None)
def _random_case(curve, n, extra=5):
    """random rs, L, R, comm, c, q, a_hat, b over a key of n + extra points, with the oracle's P_hat, G_hat and s: computed once"""
    p = field(curve)
    k = n.bit_length() - 1
    rng = random.Random(1000 * curve + n)
    gens = pasta_ref.gen_bases_ap(curve, 7, 3, n + extra)
    rs = [rng.randrange(1, p) for _ in range(k)]
    L = [_point(curve, 2 * i) for i in range(k)]
    R = [_point(curve, 2 * i + 1) for i in range(k)]
    comm, q = _point(curve, 77), affine(curve, _point(curve, 78))
    c, a_hat = rng.randrange(p), rng.randrange(p)
    b = [rng.randrange(p) for _ in range(n)]
    s = s_vector(rs, p)
    p_hat = compress(curve, msm(curve, np.stack([comm, pasta_ref.scalar_mul(curve, q, 1).reshape(12)] + L + R),
                                [1, c] + [x * x % p for x in rs] + [pow(x, -2, p) for x in rs]))
    g_hat = compress(curve, msm(curve, gens[:n], s))
    return dict(p=p, gens=gens, rs=rs, L=L, R=R, comm=comm, q=q, c=c, a_hat=a_hat, b=b, s=s, p_hat=p_hat, g_hat=g_hat)


# ------------------------------------------------------------------------------------------------ 1. intermediates
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [2, 4, 1 << 9, 1 << 13])
def test_intermediates_against_the_oracle(gpu_lib, curve, n):
    """n = 2: one round; 4: two; 2^9: more than one 256-thread block and both halves of the two-table split; 2^13: a multi-block
    reduction.  The key holds n + 5 points.  b_len in {0, 1, n - 3, n}; both forms of the scalars."""
    from reef_amd.msm import MsmContext
    from reef_amd.verify import ipa_check
    t = _random_case(curve, n)
    p = t["p"]
    with MsmContext(curve, t["gens"], bucket_groups=1) as key:
        for is_mont in (False, True):
            to, frm = _forms(p, is_mont)
            for b_len in sorted({0, 1, max(n - 3, 0), n}):
                got = ipa_check(key, n, t["comm"], to(t["c"]), t["q"], t["L"], t["R"], [to(x) for x in t["rs"]], to(t["a_hat"]),
                                [to(x) for x in t["b"][:b_len]], is_mont=is_mont, intermediates=True)
                what = f"n {n} b_len {b_len} mont {is_mont}"
                assert compress(curve, got["p_hat"]) == t["p_hat"], "P_hat " + what
                assert compress(curve, got["g_hat"]) == t["g_hat"], "G_hat " + what
                assert frm(got["b_hat"]) == dot(t["s"], pad(t["b"][:b_len], n), p), "b_hat " + what
                assert got["accept"] is False, what          # random points satisfy nothing


# ------------------------------------------------------------------------------------------------ 2. honest transcripts
def _open_case(curve, n, seed):
    p = field(curve)
    gens, gens_s = gens_of(curve, n)
    i1, i2 = random_instances(curve, n, n // 2, gens, seed)
    ref = open_ref(curve, gens, gens_s, i1, i2, Challenger(p, seed))
    b = [(x + ref["r"] * y) % p for x, y in zip(pad(i1["b"], n), pad(i2["b"], n))]
    return p, gens, gens_s, i1, i2, ref, b


@pytest.mark.parametrize("curve", [0, 1])
def test_reference_opening_transcript_accepts(gpu_lib, curve):
    from reef_amd.verify import ipa_check
    n = 32
    p, gens, gens_s, i1, i2, ref, b = _open_case(curve, n, 5 + curve)
    verify_open(curve, gens, gens_s, i1["comm"], i1["b"], i1["eval"], i2["comm"], i2["b"], i2["eval"],
                {"cross": ref["cross"], "L": ref["L"], "R": ref["R"], "a_hat": ref["a_hat"]}, Challenger(p, 5 + curve))
    with key_of_kind(curve, gens, "pre") as key:
        for is_mont in (False, True):
            to, frm = _forms(p, is_mont)
            got = ipa_check(key, n, ref["comm_a"], to(ref["c"]), ref["q"], ref["L"], ref["R"], [to(x) for x in ref["rs"]], to(ref["a_hat"]),
                            [to(x) for x in b], is_mont=is_mont, intermediates=True)
            assert got["accept"] is True and frm(got["b_hat"]) == ref["b_hat"]


def _hyrax_case(curve, num_vars, with_h, seed):
    p = field(curve)
    left = num_vars // 2
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    rng = random.Random(seed)
    point = [rng.randrange(p) for _ in range(num_vars)]
    ints = [rng.randrange(p) for _ in range((1 << num_vars) - 1)]
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)] if with_h else None
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, seed), p, h=h if with_h else None, blinds=blinds)
    comm = msm(curve, gens, ref["lz"])
    total = blind_total(0, blinds or [], ref["rs"], p)
    return dict(p=p, left=left, right=right, gens=gens, q=q, h=h if with_h else None, point=point, ints=ints, blinds=blinds, ref=ref, comm=comm,
                total=total, b0=eq_evals(point[left:], p))


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("with_h", [False, True])
def test_reference_hyrax_transcript_accepts(gpu_lib, curve, with_h):
    from reef_amd.verify import ipa_check, ipa_check_eq
    t = _hyrax_case(curve, 7, with_h, 20 + curve)
    p, ref = t["p"], t["ref"]
    verify_hyrax(curve, t["gens"], t["q"], t["comm"], ref["eval"], t["b0"], ref, p, h=t["h"], lz_blind_total=t["total"])
    kw = dict(h=t["h"], blind=t["total"]) if with_h else {}
    with key_of_kind(curve, t["gens"], "pre") as key:
        n = 1 << t["right"]
        assert ipa_check(key, n, t["comm"], ref["eval"], t["q"], ref["L"], ref["R"], ref["rs"], ref["a_hat"], t["b0"], **kw)["accept"] is True
        got = ipa_check_eq(key, n, t["comm"], ref["eval"], t["q"], ref["L"], ref["R"], ref["rs"], ref["a_hat"], [t["point"][t["left"]:]], [1],
                           intermediates=True, **kw)
        assert got["accept"] is True and got["b_hat"] == ref["b_hat"]
        if with_h:                                           # the blind term is needed: without it the same proof is refused
            assert ipa_check(key, n, t["comm"], ref["eval"], t["q"], ref["L"], ref["R"], ref["rs"], ref["a_hat"], t["b0"])["accept"] is False


def _comm_ops(curve, comm_e, comm_w, gens_s):
    def comm_a(r):
        return compress(curve, msm(curve, np.stack([comm_e, comm_w]), [1, r]))

    def q_of(r):
        return affine(curve, pasta_ref.scalar_mul(curve, gens_s, r))
    return comm_a, q_of


def _replayed(p, seed, got):
    """A challenger in the state the verifier of the opening starts from: the sum-checks' challenges re-drawn in order"""
    ch = Challenger(p, seed)
    for _ in got["tau"]:
        ch("t", [])
    for ev in got["outer"]:
        ch("outer", ev)
    ch("r", got["claims_outer"])
    for ev in got["inner"]:
        ch("inner", ev)
    return ch


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["smallest", "cons_gt_vars", "vars_gt_cons"])
def test_device_opening_transcript_through_verify_opening(gpu_lib, curve, name):
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove_with_opening
    from reef_amd.verify import verify_opening
    shape, pads = open_shape(curve, name)
    p, n = shape["p"], max(pads)
    inst = relaxed_instance(shape, 1, 11 + curve)
    gens, gens_s = gens_of(curve, n)
    E, W = list(inst["E"]), list(inst["W"])
    comm_e, comm_w = msm(curve, gens[:len(E)], E), msm(curve, gens[:len(W)], W)
    comm_a, q_of = _comm_ops(curve, comm_e, comm_w, gens_s)
    with key_of_kind(curve, gens, "pre") as key, Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        got = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 7), p, comm_a, q_of)
        eval_e, eval_w = got["claims_outer"][3], got["claims_inner"][2]
        proof = {"cross": got["cross_term"], "L": got["L"], "R": got["R"], "a_hat": got["a_hat"]}
        verify_open(curve, gens, gens_s, comm_e, eq_evals(got["r_x"], p), eval_e, comm_w, eq_evals(got["r_y"][1:], p), eval_w, proof,
                    _replayed(p, 7, got))
        assert verify_opening(key, gens_s, comm_e, got["r_x"], eval_e, comm_w, got["r_y"], eval_w, proof, _replayed(p, 7, got), p) is True
        bad = dict(proof, a_hat=(proof["a_hat"] + 1) % p)
        assert verify_opening(key, gens_s, comm_e, got["r_x"], eval_e, comm_w, got["r_y"], eval_w, bad, _replayed(p, 7, got), p) is False


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("num_vars", [2, 5, 10])
def test_device_hyrax_transcript_through_verify_eval(gpu_lib, curve, num_vars):
    from reef_amd.hyrax import HyraxEval, prove_eval
    from reef_amd._fe import _arr
    from reef_amd.verify import verify_eval
    p = field(curve)
    left = num_vars // 2
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q0, h = hyrax_points(curve)
    rng = random.Random(70 + curve + num_vars)
    point = [rng.randrange(p) for _ in range(num_vars)]
    ints = [rng.randrange(p) for _ in range((1 << num_vars) - 1)]
    rc = row_comms(curve, gens, ints, num_vars, left, None, h)
    rc32 = b"".join(compress(curve, pasta_ref.scalar_mul(curve, a, 1)) for a in rc)

    def q_of(r):
        return pasta_ref.to_affine(curve, pasta_ref.scalar_mul(curve, q0, r))[0]
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, _arr(ints), num_vars, left) as hx:
        pf = prove_eval(hx, key, point, Challenger(p, 3), p, q_of, row_comms=rc)
        q = q_of(pf["r_ipa"])
        verify_hyrax(curve, gens, q, pf["comm_lz"], pf["eval"], eq_evals(point[left:], p), pf, p)
        assert verify_eval(key, q, rc32, point, left, pf["eval"], pf, p) is True
        assert verify_eval(key, None, rc32, point, left, pf["eval"], pf, p, challenge=Challenger(p, 3), q_of=q_of) is True
        assert verify_eval(key, q, rc32, point, left, (pf["eval"] + 1) % p, pf, p) is False


# ------------------------------------------------------------------------------------------------ 3. tampers
_TAMPERS = ["L", "R", "a_hat", "c", "comm", "rs", "b", "blind", "swap"]


@pytest.mark.parametrize("curve", [0, 1])
def test_every_tamper_rejects_with_ok(gpu_lib, curve):
    """On a blinded Hyrax transcript with n = 2^9 (b has entries beyond index 256): each tamper gives REEF_OK with accept = 0, and the
    oracle's verify_hyrax raises on the same tampered input."""
    from reef_amd.verify import ipa_check
    t = _hyrax_case_wide(curve)
    p, ref = t["p"], t["ref"]
    n = 1 << t["right"]
    assert n == 512
    other = _point(curve, 5)

    def run(key, **ch):
        a = dict(comm=t["comm"], c=ref["eval"], L=list(ref["L"]), R=list(ref["R"]), rs=list(ref["rs"]), a_hat=ref["a_hat"], b=list(t["b0"]),
                 blind=t["total"])
        a.update(ch)
        got = ipa_check(key, n, a["comm"], a["c"], t["q"], a["L"], a["R"], a["rs"], a["a_hat"], a["b"], h=t["h"], blind=a["blind"])["accept"]
        try:
            verify_hyrax(curve, t["gens"], t["q"], a["comm"], a["c"], a["b"], dict(ref, L=a["L"], R=a["R"], rs=a["rs"], a_hat=a["a_hat"]), p,
                         h=t["h"], lz_blind_total=a["blind"])
            oracle = True
        except AssertionError:
            oracle = False
        return got, oracle
    with key_of_kind(curve, t["gens"], "pre") as key:
        assert run(key) == (True, True)
        i = 3
        cases = {
            "L": dict(L=ref["L"][:i] + [other] + ref["L"][i + 1:]),
            "R": dict(R=ref["R"][:i] + [other] + ref["R"][i + 1:]),
            "a_hat": dict(a_hat=(ref["a_hat"] + 1) % p),
            "c": dict(c=(ref["eval"] + 1) % p),
            "comm": dict(comm=other),
            "rs": dict(rs=ref["rs"][:i] + [(ref["rs"][i] + 1) % p] + ref["rs"][i + 1:]),
            "b": dict(b=t["b0"][:300] + [(t["b0"][300] + 1) % p] + t["b0"][301:]),
            "blind": dict(blind=(t["total"] + 1) % p),
            "swap": dict(L=list(ref["R"]), R=list(ref["L"])),
        }
        assert sorted(cases) == sorted(_TAMPERS)
        for name, ch in cases.items():
            assert run(key, **ch) == (False, False), name
        assert run(key) == (True, True)


@functools.lru_cache(maxsize=None)
def _hyrax_case_wide(curve):
    """a blinded argument over 2^9 columns from a small document: left = 1"""
    p = field(curve)
    num_vars, left = 10, 1
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    rng = random.Random(31 + curve)
    point = [rng.randrange(p) for _ in range(num_vars)]
    ints = [rng.randrange(p) for _ in range(1 << num_vars)]
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)]
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, 4), p, h=h, blinds=blinds)
    return dict(p=p, left=left, right=right, gens=gens, q=q, h=h, point=point, ref=ref, comm=msm(curve, gens, ref["lz"]),
                total=blind_total(0, blinds, ref["rs"], p), b0=eq_evals(point[left:], p))


# ------------------------------------------------------------------------------------------------ 4. key kinds
@pytest.mark.parametrize("curve", [0, 1])
def test_key_kinds_give_the_same_g_hat_and_verdict(gpu_lib, curve):
    from reef_amd.verify import ipa_check
    n = 1 << 11
    t = _random_case(curve, n, 0)
    p = t["p"]
    # an accepting input for these rs, L, R: comm chosen so that P_hat equals the right-hand side
    s = t["s"]
    b_hat = dot(s, t["b"], p)
    g_hat = msm(curve, t["gens"][:n], s)
    q_j = pasta_ref.scalar_mul(curve, t["q"], 1).reshape(12)
    comm = msm(curve, np.stack([g_hat, q_j] + t["L"] + t["R"]),
               [t["a_hat"], (t["a_hat"] * b_hat - t["c"]) % p] + [(-x * x) % p for x in t["rs"]] + [(-pow(x, -2, p)) % p for x in t["rs"]])
    for kind in ("pre", "tables", "plain"):
        with key_of_kind(curve, t["gens"], kind) as key:
            good = ipa_check(key, n, comm, t["c"], t["q"], t["L"], t["R"], t["rs"], t["a_hat"], t["b"], intermediates=True)
            assert compress(curve, good["g_hat"]) == t["g_hat"], kind
            assert good["accept"] is True and good["b_hat"] == b_hat, kind
            assert ipa_check(key, n, t["comm"], t["c"], t["q"], t["L"], t["R"], t["rs"], t["a_hat"], t["b"])["accept"] is False, kind


# ------------------------------------------------------------------------------------------------ 5. b on the device
@pytest.mark.parametrize("curve", [0, 1])
def test_check_eq_equals_check(gpu_lib, curve):
    from reef_amd._fe import _arr
    from reef_amd.msm import DeviceBuffer
    from reef_amd.verify import ipa_check, ipa_check_eq
    n = 1 << 9
    t = _random_case(curve, n)
    p = t["p"]
    rng = random.Random(9 + curve)
    p1, p2 = [rng.randrange(p) for _ in range(7)], [rng.randrange(p) for _ in range(4)]
    w = [rng.randrange(p), rng.randrange(p)]
    with key_of_kind(curve, t["gens"], "pre") as key:
        for points, weights in (([p1], w[:1]), ([p1, p2], w), ([p2, p1], w), ([[], p1], w)):
            b = [0] * n
            for pt, wt in zip(points, weights):
                for j, e in enumerate(eq_evals(pt, p) if pt else [1]):
                    b[j] = (b[j] + wt * e) % p
            blen = max(1 << len(pt) for pt in points)
            for is_mont in (False, True):
                to, frm = _forms(p, is_mont)
                args = (key, n, t["comm"], to(t["c"]), t["q"], t["L"], t["R"], [to(x) for x in t["rs"]], to(t["a_hat"]))
                a = ipa_check_eq(*args, [[to(x) for x in pt] for pt in points], [to(x) for x in weights], is_mont=is_mont, intermediates=True)
                h = ipa_check(*args, [to(x) for x in b[:blen]], is_mont=is_mont, intermediates=True)
                d = ipa_check(*args, DeviceBuffer.from_host(_arr([to(x) for x in b[:blen]])), b_len=blen, is_mont=is_mont, intermediates=True)
                assert frm(a["b_hat"]) == frm(h["b_hat"]) == frm(d["b_hat"]) == dot(t["s"], b, p)
                for x in (a, h, d):
                    assert compress(curve, x["p_hat"]) == t["p_hat"] and compress(curve, x["g_hat"]) == t["g_hat"] and x["accept"] is False


# ------------------------------------------------------------------------------------------------ 6. the comparison
@pytest.mark.parametrize("curve", [0, 1])
def test_comparison_of_identities_and_rescaled_points(gpu_lib, curve):
    from reef_amd.verify import ipa_check
    n = 4
    p = field(curve)
    gens, _ = gens_of(curve, n)
    O, Oa = np.zeros(12, np.uint64), np.zeros(8, np.uint64)
    q, h = hyrax_points(curve)
    with key_of_kind(curve, gens, "pre") as key:
        # every point the identity, a_hat = 0: identity == identity
        assert ipa_check(key, n, O, 5, Oa, [O, O], [O, O], [3, 4], 0, [1, 2, 3, 4])["accept"] is True
        # an identity left side against a non-identity right side (blind h)
        assert ipa_check(key, n, O, 5, Oa, [O, O], [O, O], [3, 4], 0, [1, 2, 3, 4], h=h, blind=1)["accept"] is False
        # and the other way round
        assert ipa_check(key, n, _point(curve, 1), 0, Oa, [O, O], [O, O], [3, 4], 0, [])["accept"] is False
    # the same points in two Jacobian scalings: L, R and comm as the prover returned them, and re-scaled by Z
    t = _hyrax_case(curve, 6, False, 12 + curve)
    ref = t["ref"]
    n = 1 << t["right"]
    with key_of_kind(curve, t["gens"], "pre") as key:
        for lam in (1, 2, 0x1234567890ABCDEF):
            L = [_rescaled(curve, x, lam) for x in ref["L"]]
            R = [_rescaled(curve, x, lam + 1) for x in ref["R"]]
            comm = _rescaled(curve, t["comm"], lam + 2)
            assert [compress(curve, x) for x in L] == [compress(curve, x) for x in ref["L"]]
            got = ipa_check(key, n, comm, ref["eval"], t["q"], L, R, ref["rs"], ref["a_hat"], t["b0"], intermediates=True)
            assert got["accept"] is True, lam
            bad = ipa_check(key, n, comm, ref["eval"], t["q"], L, R, ref["rs"], (ref["a_hat"] + 1) % p, t["b0"])
            assert bad["accept"] is False, lam


# ------------------------------------------------------------------------------------------------ 7. argument errors
@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors_change_nothing(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.verify import ipa_check, ipa_check_eq
    t = _hyrax_case(curve, 6, True, 12 + curve)
    p, ref = t["p"], t["ref"]
    n = 1 << t["right"]
    with key_of_kind(curve, t["gens"], "pre") as key:
        def call(**ch):
            a = dict(n=n, c=ref["eval"], rs=list(ref["rs"]), a_hat=ref["a_hat"], b=list(t["b0"]), h=t["h"], blind=t["total"], L=ref["L"], R=ref["R"],
                     curve=None)
            a.update(ch)
            return ipa_check(key, a["n"], t["comm"], a["c"], t["q"], a["L"], a["R"], a["rs"], a["a_hat"], a["b"], h=a["h"], blind=a["blind"],
                             curve=a["curve"])["accept"]
        assert call() is True
        k = len(ref["rs"])
        bad = [
            dict(rs=[0] + ref["rs"][1:]),                    # a zero challenge
            dict(rs=ref["rs"][:-1] + [p]),                   # a challenge that is the modulus
            dict(rs=ref["rs"][:-1] + [(1 << 256) - 1]),
            dict(c=p), dict(a_hat=p + 1), dict(blind=p), dict(b=t["b0"][:3] + [p]),      # scalars not below the modulus
            dict(n=3, L=ref["L"][:1], R=ref["R"][:1], rs=ref["rs"][:1]),
            dict(n=1, L=[], R=[], rs=[]), dict(n=0, L=[], R=[], rs=[]),
            dict(n=12, L=ref["L"][:3], R=ref["R"][:3], rs=ref["rs"][:3]),
            dict(n=2 * n, L=ref["L"] + ref["L"][:1], R=ref["R"] + ref["R"][:1], rs=ref["rs"] + [5]),   # beyond the key length
            dict(blind=None), dict(h=None),                  # h without blind, blind without h
            dict(curve=1 - curve),                           # a key of another curve: reef_amd.verify's own check (the C calls take no
                                                             # curve, the key's is the call's), raised before the library is reached
        ]
        for ch in bad:
            with pytest.raises(ReefError) as e:
                call(**ch)
            assert e.value.status == 1, ch
            assert call() is True, ch                       # nothing changed: the honest call still accepts
        with pytest.raises(ReefError):                       # eq tables larger than n, and three points
            ipa_check_eq(key, n, t["comm"], ref["eval"], t["q"], ref["L"], ref["R"], ref["rs"], ref["a_hat"], [[1] * (k + 1)], [1])
        with pytest.raises(ReefError):
            ipa_check_eq(key, n, t["comm"], ref["eval"], t["q"], ref["L"], ref["R"], ref["rs"], ref["a_hat"], [[1], [2], [3]], [1, 1, 1])
        with pytest.raises(ReefError):
            ipa_check_eq(key, n, t["comm"], ref["eval"], t["q"], ref["L"], ref["R"], ref["rs"], ref["a_hat"], [[p]], [1])
        assert call() is True
        # the outputs of a refused call are untouched
        import ctypes
        lib = key._lib
        acc = ctypes.c_uint32(7)
        out = np.full(12, 9, dtype=np.uint64)
        assert lib.reef_ipa_check(key._h, 3, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                  out.ctypes.data, None, 0, 0, None, None, False, ctypes.byref(acc), out.ctypes.data, None, None) == 1
        assert acc.value == 7 and (out == 9).all()
        assert lib.reef_ipa_check(None, 4, None, None, None, None, None, None, None, None, 0, 0, None, None, False, None, None, None, None) == 1


# ------------------------------------------------------------------------------------------------ 8. the bucket pipeline
def test_2_15_on_a_pre_shifted_key(gpu_lib):
    """n = 2^15: the size at which the bucket pipeline, not the small path, serves a pre-shifted key; G_hat against pasta_ref's Pippenger"""
    from reef_amd._fe import _arr
    from reef_amd.verify import ipa_check
    curve, n = 0, 1 << 15
    t = _random_case(curve, n, 0)
    p = t["p"]
    want = pasta_ref.compress(curve, pasta_ref.msm_pippenger(curve, np.ascontiguousarray(t["gens"][:n]), _arr(t["s"]), mont=False, threads=8))
    with key_of_kind(curve, t["gens"], "pre") as key:
        got = ipa_check(key, n, t["comm"], t["c"], t["q"], t["L"], t["R"], t["rs"], t["a_hat"], t["b"], intermediates=True)
    assert compress(curve, got["g_hat"]) == want == t["g_hat"]
    assert compress(curve, got["p_hat"]) == t["p_hat"] and got["b_hat"] == dot(t["s"], t["b"], p) and got["accept"] is False
