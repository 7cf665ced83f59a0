"""reef_ipa_check_batch on the GPU (reef_amd.verify.ipa_check_batch over include/reef_msm.h 3m) against the big-integer oracles, bit-exact
after compress: the combined vector S, both sides of the combined equation and the closed-form b_hats on random inputs at every size
and batch length where the S pass takes another path; honest batches accept; one bad proof among six is found; the weights are used;
m = 1 equals the single check; the three key kinds; the argument errors; one 2^15 case on the bucket pipeline."""
import ctypes
import functools
import random
import types

import numpy as np
import pytest

from gpu_drivers import hyrax_points, key_of_kind
from oracle import pasta_ref
from oracle.hyrax_oracle import blind_total, hyrax_ref
from oracle.ipa_oracle import affine, compress, dot, gens_of, msm, open_ref, pad, s_vector
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import Challenger, eq_evals

pytestmark = pytest.mark.gpu

_MS = (1, 2, 5, 6, 17)


def _forms(p, is_mont):
    R = (1 << 256) % p
    return ((lambda v: v * R % p), (lambda v: v * pow(R, -1, p) % p)) if is_mont else ((lambda v: v), (lambda v: v))


def _point(curve, seed):
    """a Jacobian point nobody knows a relation for"""
    return pasta_ref.scalar_mul(curve, pasta_ref.gen_bases_ap(curve, 900 + seed, 1, 1)[0], 0x1234567 + seed).reshape(12)


def _jac_of(curve, aff):
    return pasta_ref.scalar_mul(curve, aff, 1).reshape(12)


def _in_form(pr, to):
    """the proof with every scalar in the form `to` gives"""
    out = dict(pr)
    for f in ("c", "a_hat"):
        out[f] = to(pr[f])
    out["rs"] = [to(x) for x in pr["rs"]]
    out["points"] = [[to(x) for x in pt] for pt in pr["points"]]
    out["weights"] = [to(x) for x in pr["weights"]]
    if pr.get("blind") is not None:
        out["blind"] = to(pr["blind"])
    return out


def _b_of(pr, n, p):
    b = [0] * n
    for pt, w in zip(pr["points"], pr["weights"]):
        for j, e in enumerate(eq_evals(pt, p) if pt else [1]):
            b[j] = (b[j] + w * e) % p
    return b


def _one_off(curve, proofs, rho, b_hats, p):
    """the points and scalars of the left side of the combined equation"""
    pts, ks = [], []
    for pr, r, bh in zip(proofs, rho, b_hats):
        pts += [pr["comm"], _jac_of(curve, pr["q"])] + list(pr["L"]) + list(pr["R"])
        ks += [r, r * (pr["c"] - pr["a_hat"] * bh) % p] + [r * x * x % p for x in pr["rs"]] + [r * pow(x, -2, p) % p for x in pr["rs"]]
        if pr.get("h") is not None:
            pts.append(_jac_of(curve, pr["h"]))
            ks.append(-r * pr["blind"] % p)
    return np.stack(pts), ks


def _msm_big(curve, gens, scalars):
    from reef_amd._fe import _arr
    return pasta_ref.msm_pippenger(curve, np.ascontiguousarray(gens), _arr(scalars), mont=False, threads=8)


@functools.lru_cache(maxsize=None)
def _random_batch(curve, n, m_max=max(_MS), extra=5):
    """m_max random proofs over a key of n + extra points and, for every m of _MS, the oracle's S, both sides and b_hats: computed once"""
    p = field(curve)
    k = n.bit_length() - 1
    rng = random.Random(5000 * curve + n)
    gens = pasta_ref.gen_bases_ap(curve, 7, 3, n + extra)
    pool = [_point(curve, i) for i in range(2 * k + 2)]
    proofs, rho, ss, b_hats = [], [], [], []
    for i in range(m_max):
        rs = [rng.randrange(1, p) for _ in range(k)]
        pick = [pool[(i + j) % len(pool)] for j in range(2 * k + 2)]        # the same few points in another order per proof
        vs = [k] if i % 3 == 0 else ([k // 2, k - 1] if i % 3 == 1 else [0, k])
        pr = dict(comm=pick[0], q=affine(curve, pick[1]), L=pick[2:2 + k], R=pick[2 + k:], rs=rs, c=rng.randrange(p), a_hat=rng.randrange(p),
                  points=[[rng.randrange(p) for _ in range(v)] for v in vs], weights=[rng.randrange(p) for _ in vs])
        if i % 4 == 1:
            pr.update(h=hyrax_points(curve)[1], blind=rng.randrange(p))
        s = s_vector(rs, p)
        proofs.append(pr)
        rho.append(rng.randrange(1, p))
        ss.append(s)
        b_hats.append(dot(s, _b_of(pr, n, p), p))
    want, S = {}, [0] * n
    for m in range(1, m_max + 1):
        w = rho[m - 1] * proofs[m - 1]["a_hat"] % p
        S = [(x + w * y) % p for x, y in zip(S, ss[m - 1])]
        if m in _MS:
            pts, ks = _one_off(curve, proofs[:m], rho[:m], b_hats[:m], p)
            want[m] = dict(S=S, g=compress(curve, _msm_big(curve, gens[:n], S)), d=compress(curve, msm(curve, pts, ks)))
    return dict(p=p, gens=gens, proofs=proofs, rho=rho, b_hats=b_hats, want=want)


# ------------------------------------------------------------------------------------------------ 1. intermediates
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [2, 4, 1 << 9, 1 << 13])
def test_intermediates_against_the_oracle(gpu_lib, curve, n):
    """n = 2: one round; 4: two; 2^9: more than one block and both halves of the table split; 2^13: multi-block, and a wave shares its
    hi entry.  m = 5 and 6 straddle a five-product lazy reduction, 17 spans several groups.  The key holds n + 5 points; both forms."""
    from reef_amd.msm import DeviceBuffer, MsmContext
    from reef_amd._fe import _ints
    from reef_amd.verify import ipa_check_batch
    t = _random_batch(curve, n)
    p = t["p"]
    with MsmContext(curve, t["gens"], bucket_groups=1) as key:
        for m in _MS:
            w = t["want"][m]
            for is_mont in (False, True):
                to, frm = _forms(p, is_mont)
                got = ipa_check_batch(key, n, [_in_form(pr, to) for pr in t["proofs"][:m]], [to(x) for x in t["rho"][:m]], is_mont=is_mont,
                                      intermediates=True)
                what = f"n {n} m {m} mont {is_mont}"
                assert got["s_comb"] == w["S"], "S " + what
                assert compress(curve, got["g_comb"]) == w["g"], "g_comb " + what
                assert compress(curve, got["d_comb"]) == w["d"], "d_comb " + what
                assert [frm(x) for x in got["b_hats"]] == t["b_hats"][:m], "b_hats " + what
                assert got["accept"] is False, what          # random points satisfy nothing
            d_s = DeviceBuffer(32 * n)
            got = ipa_check_batch(key, n, t["proofs"][:m], t["rho"][:m], s_comb_out=d_s)
            assert _ints(d_s.to_host((n, 4))) == w["S"] and got["accept"] is False, f"device S n {n} m {m}"


# ------------------------------------------------------------------------------------------------ 2. honest batches
@functools.lru_cache(maxsize=None)
def _hyrax_proof(curve, num_vars, with_h, seed):
    """a Hyrax transcript of the reference prover as a proof of a batch, and its b_hat"""
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
    pr = dict(comm=msm(curve, gens, ref["lz"]), c=ref["eval"], q=q, L=list(ref["L"]), R=list(ref["R"]), rs=list(ref["rs"]), a_hat=ref["a_hat"],
              points=[point[left:]], weights=[1])
    if with_h:
        pr.update(h=h, blind=blind_total(0, blinds, ref["rs"], p))
    return pr, ref["b_hat"]


def _hyrax_batch(curve, count, blinded, num_vars=7):
    got = [_hyrax_proof(curve, num_vars, i in blinded, 40 + 7 * i + curve) for i in range(count)]
    return [dict(pr) for pr, _ in got], [bh for _, bh in got]


@functools.lru_cache(maxsize=None)
def _opening_proof(curve, n, seed):
    """an opening of the reference prover over two instances whose b vectors are eq tables: the two-point eq form"""
    p = field(curve)
    gens, gens_s = gens_of(curve, n)
    rng = random.Random(seed)
    k = n.bit_length() - 1
    r_x, r_y = [rng.randrange(p) for _ in range(k)], [rng.randrange(p) for _ in range(k - 1)]
    insts = []
    for pt in (r_x, r_y):
        b = eq_evals(pt, p)
        a = [rng.randrange(p) for _ in range(len(b) - 1)]
        insts.append({"a": a, "b": b, "comm": msm(curve, gens[:len(a)], a), "eval": dot(a, b, p)})
    ref = open_ref(curve, gens, gens_s, insts[0], insts[1], Challenger(p, seed))
    pr = dict(comm=ref["comm_a"], c=ref["c"], q=ref["q"], L=list(ref["L"]), R=list(ref["R"]), rs=list(ref["rs"]), a_hat=ref["a_hat"],
              points=[r_x, r_y], weights=[1, ref["r"]])
    return pr, ref["b_hat"]


def _rho(p, m, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, p) for _ in range(m)]


@pytest.mark.parametrize("curve", [0, 1])
def test_honest_batches_accept(gpu_lib, curve):
    from reef_amd.verify import ipa_check_batch
    p = field(curve)
    proofs, b_hats = _hyrax_batch(curve, 5, {1, 3})
    with key_of_kind(curve, gens_of(curve, 16)[0], "pre") as key:
        for is_mont in (False, True):
            to, frm = _forms(p, is_mont)
            got = ipa_check_batch(key, 16, [_in_form(pr, to) for pr in proofs], [to(x) for x in _rho(p, 5, 1)], is_mont=is_mont, each=True,
                                  intermediates=True)
            assert got["accept"] is True and got["each"] == [True] * 5
            assert [frm(x) for x in got["b_hats"]] == b_hats
    opened = [_opening_proof(curve, 32, 60 + i + curve) for i in range(3)]
    with key_of_kind(curve, gens_of(curve, 32)[0], "pre") as key:
        got = ipa_check_batch(key, 32, [pr for pr, _ in opened], _rho(p, 3, 2), each=True, intermediates=True)
        assert got["accept"] is True and got["each"] == [True] * 3 and got["b_hats"] == [bh for _, bh in opened]


# ------------------------------------------------------------------------------------------------ 3. one bad among six
_TAMPERS = ["L", "R", "a_hat", "c", "comm", "rs", "point", "blind", "swap"]


def _tampered(curve, pr, name, p):
    other, i = _point(curve, 5), 3
    ch = {
        "L": lambda: dict(L=pr["L"][:i] + [other] + pr["L"][i + 1:]),
        "R": lambda: dict(R=pr["R"][:i] + [other] + pr["R"][i + 1:]),
        "a_hat": lambda: dict(a_hat=(pr["a_hat"] + 1) % p),
        "c": lambda: dict(c=(pr["c"] + 1) % p),
        "comm": lambda: dict(comm=other),
        "rs": lambda: dict(rs=pr["rs"][:i] + [(pr["rs"][i] + 1) % p] + pr["rs"][i + 1:]),
        "point": lambda: dict(points=[pr["points"][0][:2] + [(pr["points"][0][2] + 1) % p] + pr["points"][0][3:]]),
        "blind": lambda: dict(blind=(pr["blind"] + 1) % p),
        "swap": lambda: dict(L=list(pr["R"]), R=list(pr["L"])),
    }[name]()
    return dict(pr, **ch)


@pytest.mark.parametrize("curve", [0, 1])
def test_one_bad_proof_among_six_is_found(gpu_lib, curve):
    from reef_amd.verify import ipa_check_batch
    p = field(curve)
    proofs, _ = _hyrax_batch(curve, 6, {1, 3})               # proof 3 is blinded: every tamper applies to it
    assert len(proofs[3]["rs"]) == 4 and proofs[3].get("blind") is not None
    rho = _rho(p, 6, 3)
    with key_of_kind(curve, gens_of(curve, 16)[0], "pre") as key:
        assert ipa_check_batch(key, 16, proofs, rho, each=True) == {"accept": True, "each": [True] * 6}
        for name in _TAMPERS:
            bad = proofs[:3] + [_tampered(curve, proofs[3], name, p)] + proofs[4:]
            got = ipa_check_batch(key, 16, bad, rho, each=True)
            assert got == {"accept": False, "each": [True, True, True, False, True, True]}, name
            assert ipa_check_batch(key, 16, bad, rho) == {"accept": False}, name          # accept_each NULL: only the verdict
        assert ipa_check_batch(key, 16, proofs, rho, each=True) == {"accept": True, "each": [True] * 6}


# ------------------------------------------------------------------------------------------------ 4. the weights
@pytest.mark.parametrize("curve", [0, 1])
def test_the_weights_are_used(gpu_lib, curve):
    """comm_0 + X beside comm_1 - X: rho = [1, 1] accepts -- that is what the equation says, the weights are the caller's -- and
    rho = [1, 2] rejects; neither proof verifies alone."""
    from reef_amd.verify import ipa_check_batch
    p = field(curve)
    proofs, _ = _hyrax_batch(curve, 2, {1})
    X = _point(curve, 9)
    proofs[0]["comm"] = msm(curve, np.stack([proofs[0]["comm"], X]), [1, 1])
    proofs[1]["comm"] = msm(curve, np.stack([proofs[1]["comm"], X]), [1, p - 1])
    with key_of_kind(curve, gens_of(curve, 16)[0], "pre") as key:
        assert ipa_check_batch(key, 16, proofs, [1, 1])["accept"] is True
        assert ipa_check_batch(key, 16, proofs, [1, 2], each=True) == {"accept": False, "each": [False, False]}


# ------------------------------------------------------------------------------------------------ 5. m = 1
@pytest.mark.parametrize("curve", [0, 1])
def test_a_batch_of_one_equals_the_single_check(gpu_lib, curve):
    from reef_amd.verify import ipa_check_batch, ipa_check_eq
    p = field(curve)
    proofs, _ = _hyrax_batch(curve, 4, {1, 3})
    honest = proofs[3]
    with key_of_kind(curve, gens_of(curve, 16)[0], "pre") as key:
        for name in [None] + _TAMPERS:
            pr = honest if name is None else _tampered(curve, honest, name, p)
            one = ipa_check_eq(key, 16, pr["comm"], pr["c"], pr["q"], pr["L"], pr["R"], pr["rs"], pr["a_hat"], pr["points"], pr["weights"], h=pr["h"],
                               blind=pr["blind"], intermediates=True)
            got = ipa_check_batch(key, 16, [pr], [1], each=True, intermediates=True)
            assert got["accept"] is one["accept"] is (name is None), name
            assert got["each"] == [one["accept"]] and got["b_hats"] == [one["b_hat"]], name


# ------------------------------------------------------------------------------------------------ 6. key kinds
@pytest.mark.parametrize("curve", [0, 1])
def test_key_kinds_give_the_same_g_comb_and_verdict(gpu_lib, curve):
    from reef_amd.verify import ipa_check_batch
    n, m = 1 << 11, 3
    p = field(curve)
    k = n.bit_length() - 1
    rng = random.Random(77 + curve)
    gens = pasta_ref.gen_bases_ap(curve, 7, 3, n)
    pool = [_point(curve, i) for i in range(2 * k + 2)]
    proofs, rho, S = [], _rho(p, m, 4), [0] * n
    for i in range(m):
        rs = [rng.randrange(1, p) for _ in range(k)]
        pr = dict(comm=pool[i], q=affine(curve, pool[(i + 1) % len(pool)]), L=pool[2:2 + k], R=pool[2 + k:], rs=rs, c=rng.randrange(p),
                  a_hat=rng.randrange(p), points=[[rng.randrange(p) for _ in range(k - i)]], weights=[rng.randrange(p)])
        w = rho[i] * pr["a_hat"] % p
        S = [(x + w * y) % p for x, y in zip(S, s_vector(rs, p))]
        proofs.append(pr)
    from reef_amd.verify import eq_b_hat
    b_hats = [eq_b_hat(pr["rs"], pr["points"], pr["weights"], p) for pr in proofs]
    g = _msm_big(curve, gens, S)
    # an accepting input for these proofs: comm_0 chosen so that the combined equation holds
    pts, ks = _one_off(curve, proofs, rho, b_hats, p)
    inv0 = pow(rho[0], -1, p)
    good0 = msm(curve, np.vstack([g[None], pts[1:]]), [inv0] + [(-x * inv0) % p for x in ks[1:]])
    good = [dict(proofs[0], comm=good0)] + proofs[1:]
    for kind in ("pre", "tables", "plain"):
        with key_of_kind(curve, gens, kind) as key:
            got = ipa_check_batch(key, n, good, rho, intermediates=True)
            assert compress(curve, got["g_comb"]) == compress(curve, g), kind
            assert got["accept"] is True and got["b_hats"] == b_hats, kind
            assert ipa_check_batch(key, n, proofs, rho)["accept"] is False, kind


# ------------------------------------------------------------------------------------------------ 7. argument errors
def _raw(key, n, proofs, rho):
    """the C call with every output a sentinel: (status, outputs untouched)"""
    from reef_amd.verify import _marshal_batch
    structs, ra, keep = _marshal_batch(n, proofs, rho)
    m = len(proofs)
    acc = ctypes.c_uint32(7)
    each = (ctypes.c_uint32 * m)(*([9] * m))
    bh, sc = np.full((m, 4), 9, np.uint64), np.full((max(n, 1), 4), 9, np.uint64)
    dg = np.full((2, 12), 9, np.uint64)
    st = key._lib.reef_ipa_check_batch(key._h, n, structs, m, ra.ctypes.data, False, ctypes.byref(acc), ctypes.cast(each, ctypes.c_void_p), bh.ctypes.data,
                                       sc.ctypes.data, 0, dg[0].ctypes.data, dg[1].ctypes.data)
    del keep
    return st, acc.value == 7 and list(each) == [9] * m and (bh == 9).all() and (sc == 9).all() and (dg == 9).all()


@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors_change_nothing(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.msm import DeviceBuffer
    from reef_amd.verify import ipa_check, ipa_check_batch
    p = field(curve)
    n, k = 16, 4
    proofs, _ = _hyrax_batch(curve, 3, {1})
    rho = _rho(p, 3, 5)
    gens = gens_of(curve, 16)[0]

    def with_proof(i, **ch):
        return proofs[:i] + [dict(proofs[i], **ch)] + proofs[i + 1:]
    with key_of_kind(curve, gens, "pre") as key:
        honest = lambda: ipa_check_batch(key, n, proofs, rho, each=True) == {"accept": True, "each": [True] * 3}
        assert honest()
        two = lambda pr: dict(pr, L=pr["L"][:1], R=pr["R"][:1], rs=pr["rs"][:1])
        seven = dict(proofs[0], L=proofs[0]["L"] + proofs[0]["L"][:3], R=proofs[0]["R"] + proofs[0]["R"][:3], rs=proofs[0]["rs"] + [5, 6, 7])
        bad = [
            (n, proofs, [rho[0], 0, rho[2]]), (n, proofs, [p] + rho[1:]), (n, proofs, rho[:2] + [(1 << 256) - 1]),
            (n, with_proof(2, points=[], weights=[]), rho), (n, with_proof(0, points=[[1], [2], [3]], weights=[1, 1, 1]), rho),
            (n, with_proof(1, points=[[1] * (k + 1)]), rho),                                  # vars > k
            (n, with_proof(1, blind=None), rho), (n, with_proof(1, h=None), rho),             # h without blind, blind without h
            (n, with_proof(2, rs=[0] + proofs[2]["rs"][1:]), rho), (n, with_proof(0, c=p), rho), (n, with_proof(0, a_hat=p + 1), rho),
            (2 * n, [dict(pr, L=pr["L"] + pr["L"][:1], R=pr["R"] + pr["R"][:1], rs=pr["rs"] + [5]) for pr in proofs], rho),   # beyond the key
            (3, [two(pr) for pr in proofs], rho),
            (2, [two(proofs[0])] * 4097, [1] * 4097),                                         # m over 4096 (4097 * 5 points are within 2^16)
            (128, [seven] * 4096, [1] * 4096),                                                # 4096 * 17 one-off points: over 2^16
        ]
        for nn, prs, rh in bad:
            st, untouched = _raw(key, nn, prs, rh)
            assert st == 1 and untouched, (nn, len(prs), key._lib.reef_last_error())
            assert honest()
        st, _ = _raw(key, n, with_proof(2, c=p), rho)
        assert st == 1 and b"proof 2" in key._lib.reef_last_error()                           # the message names the proof ...
        st, _ = _raw(key, 128, [seven] * 4096, [1] * 4096)
        assert st == 1 and b"4096" in key._lib.reef_last_error() and str(4096 * 17).encode() in key._lib.reef_last_error()   # ... and both numbers
        # a null field of a proof
        from reef_amd.verify import _marshal_batch
        structs, ra, keep = _marshal_batch(n, proofs, rho)
        structs[1].rs = None
        acc = ctypes.c_uint32(7)
        assert key._lib.reef_ipa_check_batch(key._h, n, structs, 3, ra.ctypes.data, False, ctypes.byref(acc), None, None, None, 0, None, None) == 1
        assert acc.value == 7 and b"proof 1" in key._lib.reef_last_error()
        assert honest()
        # a window split on the key ctx
        key.set_window_split(0, 2)
        st, untouched = _raw(key, n, proofs, rho)
        assert st == 1 and untouched
        key.set_window_split(0, 1)
        assert honest()
        # a misaligned device s_comb
        d_s = DeviceBuffer(32 * n + 16)
        with pytest.raises(ReefError) as e:
            ipa_check_batch(key, n, proofs, rho, s_comb_out=types.SimpleNamespace(ptr=d_s.ptr + 8, nbytes=32 * n))
        assert e.value.status == 1
        assert honest()
        # the 64-slot side key of the single calls is intact: the same P_hat, G_hat and verdict before and after a 40-proof batch
        pr = proofs[1]
        single = lambda: ipa_check(key, n, pr["comm"], pr["c"], pr["q"], pr["L"], pr["R"], pr["rs"], pr["a_hat"], eq_evals(pr["points"][0], p),
                                   h=pr["h"], blind=pr["blind"], intermediates=True)
        before = single()
        forty = [proofs[i % 3] for i in range(40)]
        assert ipa_check_batch(key, n, forty, _rho(p, 40, 6), each=True) == {"accept": True, "each": [True] * 40}
        after = single()
        assert before["accept"] is after["accept"] is True and before["b_hat"] == after["b_hat"]
        assert compress(curve, before["p_hat"]) == compress(curve, after["p_hat"]) and compress(curve, before["g_hat"]) == compress(curve, after["g_hat"])


# ------------------------------------------------------------------------------------------------ 8. the bucket pipeline
def test_2_15_on_a_pre_shifted_key(gpu_lib):
    """Pallas, n = 2^15, m = 4: the size at which the bucket pipeline, not the small path, serves a pre-shifted key"""
    from reef_amd.verify import eq_b_hat, ipa_check_batch
    curve, n, m = 0, 1 << 15, 4
    p = field(curve)
    k = 15
    rng = random.Random(15)
    gens = pasta_ref.gen_bases_ap(curve, 7, 3, n)
    pool = [_point(curve, i) for i in range(2 * k + 2)]
    proofs, rho, S = [], _rho(p, m, 7), [0] * n
    for i in range(m):
        rs = [rng.randrange(1, p) for _ in range(k)]
        pr = dict(comm=pool[i], q=affine(curve, pool[i + 1]), L=pool[2:2 + k], R=pool[2 + k:], rs=rs, c=rng.randrange(p), a_hat=rng.randrange(p),
                  points=[[rng.randrange(p) for _ in range(k)], [rng.randrange(p) for _ in range(k - 1)]], weights=[1, rng.randrange(p)])
        w = rho[i] * pr["a_hat"] % p
        S = [(x + w * y) % p for x, y in zip(S, s_vector(rs, p))]
        proofs.append(pr)
    b_hats = [eq_b_hat(pr["rs"], pr["points"], pr["weights"], p) for pr in proofs]
    pts, ks = _one_off(curve, proofs, rho, b_hats, p)
    with key_of_kind(curve, gens, "pre") as key:
        got = ipa_check_batch(key, n, proofs, rho, intermediates=True)
    assert got["s_comb"] == S
    assert compress(curve, got["g_comb"]) == pasta_ref.compress(curve, _msm_big(curve, gens, S))
    assert compress(curve, got["d_comb"]) == compress(curve, msm(curve, pts, ks)) and got["b_hats"] == b_hats and got["accept"] is False


# ------------------------------------------------------------------------------------------------ 9. verify_eval_batch
@pytest.mark.parametrize("curve", [0, 1])
def test_device_hyrax_transcripts_through_verify_eval_batch(gpu_lib, curve):
    """Three arguments of the device prover over the same gens_v, verified in one pass; the weights come from the caller's callable,
    which sees what every proof contributes; one wrong evaluation is found."""
    from gpu_drivers import row_comms
    from reef_amd._fe import _arr
    from reef_amd.hyrax import HyraxEval, prove_eval
    from reef_amd.verify import verify_eval_batch
    p = field(curve)
    num_vars, left = 6, 3
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q0, h = hyrax_points(curve)

    def q_of(r):
        return pasta_ref.to_affine(curve, pasta_ref.scalar_mul(curve, q0, r))[0]
    seen = []

    def weights(absorbed):
        seen.append(absorbed)
        ch = Challenger(p, 99)
        return [ch("rho", item) or 1 for item in absorbed]
    with key_of_kind(curve, gens, "pre") as key:
        insts = []
        for i in range(3):
            rng = random.Random(300 + 10 * curve + i)
            point = [rng.randrange(p) for _ in range(num_vars)]
            ints = [rng.randrange(p) for _ in range((1 << num_vars) - 1)]
            rc = row_comms(curve, gens, ints, num_vars, left, None, h)
            rc32 = b"".join(compress(curve, pasta_ref.scalar_mul(curve, a, 1)) for a in rc)
            with HyraxEval(curve, _arr(ints), num_vars, left) as hx:
                pf = prove_eval(hx, key, point, Challenger(p, 3 + i), p, q_of, row_comms=rc)
            # the first one re-draws its challenges, the others bring them
            insts.append(dict(q=None, row_comms32=rc32, point=point, left=left, eval=pf["eval"], proof=pf, challenge=Challenger(p, 3), q_of=q_of) if i == 0
                         else dict(q=q_of(pf["r_ipa"]), row_comms32=rc32, point=point, left=left, eval=pf["eval"], proof=pf))
        assert verify_eval_batch(key, insts, p, weights) is True
        assert len(seen) == 1 and len(seen[0]) == 3 and all(len(item) == 3 + 2 * right for item in seen[0])
        insts[0]["challenge"] = Challenger(p, 3)
        assert verify_eval_batch(key, insts, p, weights, each=True) == (True, [True] * 3)
        bad = insts[:1] + [dict(insts[1], eval=(insts[1]["eval"] + 1) % p)] + insts[2:]
        bad[0] = dict(bad[0], challenge=Challenger(p, 3))
        assert verify_eval_batch(key, bad, p, weights, each=True) == (False, [True, False, True])
        bad[0] = dict(bad[0], challenge=Challenger(p, 3))
        assert verify_eval_batch(key, bad, p, weights) is False
        assert verify_eval_batch(key, [], p, weights) is True
