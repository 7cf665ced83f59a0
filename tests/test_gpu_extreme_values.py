"""Worst-case values through the rows that accumulate lazily (fe_vec.h: wide18_mac, fe_from_limb_sums, wave_sum63), each against
its family's Python reference, bit-exactly.  The row parity tests draw uniform entries, whose table forms have top limbs near
2^21 and whose lane and column sums stay far below the stated limits; here every entry is
  canonical max  M - 1,
  table max      the integer whose internal form x 2^261 mod M is 2^254 - 1 (limbs 0..7 at 2^29 - 1, the top limb at 2^22 - 1),
  mixed          those two alternating with 0 and 1,
and the challenges are M - 1 or the table max.  The inputs need not satisfy any relation: only transcripts are compared.
Every test but the last (pure Python: the extreme values are what they claim) needs the GPU."""

import pytest

from merkle_drivers import table_max
from oracle import mle_oracle
from oracle.pasta_oracle import CURVES, P, Q
from oracle.sumcheck_oracle import gen_eq_table, linear_mle_coeffs, linear_mle_fold

R256 = 1 << 256


def values(kind, mod, n):
    t = table_max(mod)
    if kind == "canonical_max":
        return [mod - 1] * n
    if kind == "table_max":
        return [t] * n
    return [(mod - 1, 0, t, 1)[i % 4] for i in range(n)]


KINDS = ["canonical_max", "table_max", "mixed"]


# ------------------------------------------------------------------------------------------------------- N2 sum-check ----

@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fused", [False, True])
def test_sumcheck_extremes(curve, kind, fused, gpu_lib):
    """Tables and eq at the extremes, every round and fold, challenges M - 1 and table max; the plain and the one-launch path."""
    from reef_amd.sumcheck import SumCheck
    q = CURVES[curve].order
    ell = 11
    t = values(kind, q, 1 << ell)
    e = values(KINDS[(KINDS.index(kind) + 1) % 3], q, 1 << ell)
    rs = [q - 1 if i % 2 else table_max(q) for i in range(ell)]
    with SumCheck(curve, ell) as sc:
        sc.set_table(0, t)
        sc.set_table(1, e)
        g = sc.round_coeffs(1)
        for i in range(1, ell + 1):
            assert g == linear_mle_coeffs(t, e, ell, i, q), i
            linear_mle_fold(t, e, ell, i, rs[i - 1], q)
            if fused and i < ell:
                g = sc.fold_and_next_coeffs(i, rs[i - 1])
            else:
                sc.fold(i, rs[i - 1])
                if i < ell:
                    g = sc.round_coeffs(i + 1)
            assert sc.read(0, 1 << (ell - i)) == t[: 1 << (ell - i)], i
            assert sc.read(1, 1 << (ell - i)) == e[: 1 << (ell - i)], i


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_sumcheck_eq_inputs_at_extremes(curve, gpu_lib):
    """The device-generated eq table with every input at M - 1 or table max, then every round."""
    from reef_amd.sumcheck import SumCheck
    q = CURVES[curve].order
    ell = 10
    t = values("mixed", q, 1 << ell)
    qs = [(1 << ell) - 1, 0, 5, 5]
    rs = [q - 1, table_max(q), q - 1, table_max(q), q - 1]
    last_q = [q - 1 if i % 2 else table_max(q) for i in range(ell)]
    e = gen_eq_table(rs, qs, last_q, q)
    with SumCheck(curve, ell) as sc:
        sc.set_table(0, t)
        sc.gen_eq_table(rs, qs, last_q)
        assert sc.read(1, 1 << ell) == e
        for i in range(1, ell + 1):
            assert sc.round_coeffs(i) == linear_mle_coeffs(t, e, ell, i, q), i
            sc.fold(i, q - 1)
            linear_mle_fold(t, e, ell, i, q - 1, q)


# ----------------------------------------------------------------------------------------------------------- N3 MLE ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pallas", "vesta"])
@pytest.mark.parametrize("is_mont", [False, True])
@pytest.mark.parametrize("m,left", [(10, 5), (12, 2)])
def test_mle_field_documents_at_extremes(name, is_mont, m, left, gpu_lib):
    """32-byte entries enter wide18_mac raw: the worst entry reads 2^254 - 1 in the form given; M - 1 and table max as well."""
    from reef_amd import mle
    from reef_amd.sumcheck import array_to_ints, ints_to_array
    mod = {"pallas": Q, "vesta": P}[name]
    raw = [(1 << 254) - 1, mod - 1, (1 << 254) - 1, table_max(mod), 0, 1]
    words = [raw[i % len(raw)] if i % 7 else (1 << 254) - 1 for i in range(1 << m)]
    z = [w * pow(R256, -1, mod) % mod for w in words] if is_mont else words
    point = [mod - 1 if i % 2 else table_max(mod) for i in range(m)]
    lz_ref, ev_ref = mle_oracle.bound_rows(z, point, left, mod)
    pt = ints_to_array([v * R256 % mod for v in point] if is_mont else point)
    lz, ev = mle.bound_rows_raw(name, ints_to_array(words), pt, left, is_mont=is_mont)
    scale = R256 if is_mont else 1
    assert array_to_ints(ev)[0] == ev_ref * scale % mod
    assert array_to_ints(lz) == [v * scale % mod for v in lz_ref]


# --------------------------------------------------------------------------------------------------------- N5 Spartan ----

def _extreme_instance(shape, kind):
    p = shape["p"]
    nv, ni = shape["num_vars"], shape["num_io"]
    return {"W": values(kind, p, nv), "E": values(KINDS[(KINDS.index(kind) + 2) % 3], p, shape["num_cons"]),
            "X": values(kind, p, ni), "u": p - 1 if kind != "table_max" else table_max(p)}


def _extreme_coefficients(shape):
    """General coefficients at M - 1 and table max (every third entry keeps its small value)."""
    p, out = shape["p"], dict(shape)
    for k in "ABC":
        r, c, v = shape[k]
        out[k] = (list(r), list(c), [x if i % 3 == 0 else (p - 1 if i % 2 else table_max(p)) for i, x in enumerate(v)])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["smallest", "dup_empty"])
@pytest.mark.parametrize("kind", KINDS)
def test_spartan_extremes(gpu_lib, curve, name, kind):
    from reef_amd.nifs import Nifs
    from gpu_drivers import PROOF_KEYS, prove_dev, set_running, spartan_shape, upload_shape
    from oracle.spartan_oracle import Challenger, prove_ref
    shape, pads = spartan_shape(curve, name)
    shape = _extreme_coefficients(shape)
    p = shape["p"]
    inst = _extreme_instance(shape, kind)
    ref = prove_ref(shape, inst, pads[0], pads[1], Challenger(p, curve), strict=False)
    for is_mont in (False, True):
        with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
            upload_shape(nf, shape, is_mont)
            set_running(nf, inst, p, is_mont)
            got = prove_dev(nf, shape, pads, is_mont, curve)
            for k in PROOF_KEYS:
                assert got[k] == ref[k], f"{k} ({'Montgomery' if is_mont else 'canonical'} form)"


# ------------------------------------------------------------------------------------------------------------ N6 NIFS ----

NIFS_LONG_ROW = 128   # nifs_kernels.inc: rows with more entries (A + B + C) are cut into segments of a block each
COEFS = [0xFFFF, -0xFFFF, 0x10000, -0x10000, -1, 1]   # the largest small magnitude, the smallest general one, and -1 / 1


def _nifs_shape(curve):
    """Rows of 700 (several long-row segments), 128 (the longest short row), 129 (the shortest long one), 3 and 0 entries;
    coefficients +-0xFFFF, +-0x10000, -1, 1 and table max."""
    from oracle.r1cs_oracle import field
    p = field(curve)
    num_vars, num_io = 400, 2
    ncols = num_vars + 1 + num_io
    coefs = [c % p for c in COEFS] + [table_max(p)]
    mats = {k: ([], [], []) for k in "ABC"}
    k = 0
    for row, (na, nb, nc) in enumerate([(300, 200, 200), (64, 32, 32), (65, 32, 32), (1, 1, 1), (0, 0, 0)]):
        for mat, cnt in zip("ABC", (na, nb, nc)):
            for j in range(cnt):
                mats[mat][0].append(row)
                mats[mat][1].append((row * 131 + j * 7 + "ABC".index(mat)) % ncols)
                mats[mat][2].append(coefs[k % len(coefs)])
                k += 1
    assert [sum(r.count(i) for r in (mats[m][0] for m in "ABC")) for i in range(3)] == [700, NIFS_LONG_ROW, NIFS_LONG_ROW + 1]
    return {"num_cons": 5, "num_vars": num_vars, "num_io": num_io, "p": p, **mats}


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_nifs_extremes(gpu_lib, curve, kind):
    """T = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - CZ1 and the fold with r = M - 1, both input forms, z at the extremes."""
    from reef_amd.msm import compress
    from reef_amd.nifs import E, T, U, W, X, Nifs
    from gpu_drivers import ap_key, arr, set_running, upload_shape
    from oracle import pasta_ref as R
    from oracle.r1cs_oracle import cross_term, fold, to_mont
    from reef_amd._fe import _arr, _ints
    shape = _nifs_shape(curve)
    p, n = shape["p"], shape["num_cons"]
    other = KINDS[(KINDS.index(kind) + 1) % 3]
    run = {"W": values(kind, p, shape["num_vars"]), "E": values(other, p, n), "u": table_max(p) if kind == "table_max" else p - 1,
           "X": values(kind, p, shape["num_io"])}
    fresh = {"W": values(kind, p, shape["num_vars"])[::-1], "X": values(other, p, shape["num_io"])}
    t_ref = cross_term(shape, run, fresh, p)
    r = p - 1
    ref = fold(run, fresh, t_ref, r, p)
    bases, key = ap_key(curve, n)
    with key:
        for is_mont in (False, True):
            form = "Montgomery" if is_mont else "canonical"
            with Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
                upload_shape(nf, shape, is_mont)
                set_running(nf, run, p, is_mont)
                comm = nf.commit_t(key, arr(fresh["W"], p, is_mont), arr(fresh["X"], p, is_mont), is_mont=is_mont)
                assert _ints(nf.read(T)) == t_ref, f"T ({form})"
                if not is_mont:
                    assert compress(curve, comm) == R.compress(curve, R.msm_pippenger(curve, bases, _arr(t_ref), mont=False, threads=4))
                nf.fold(to_mont([r], p)[0] if is_mont else r, is_mont=is_mont)
                got = {"W": _ints(nf.read(W)), "E": _ints(nf.read(E)), "u": _ints(nf.read(U))[0], "X": _ints(nf.read(X))}
                assert got == ref, f"fold ({form})"


# ---------------------------------------------------------------------------------------------- the batched IPA opening ----

@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_opening_extremes(gpu_lib, curve, kind):
    """a = E and W at the extremes (b follows from the reference's challenges), both input forms, every round."""
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove
    from gpu_drivers import key_of_kind, opening_instances, run_opening, set_running, spartan_shape, upload_shape
    from oracle.ipa_oracle import gens_of, open_ref
    from oracle.spartan_oracle import Challenger, prove_ref
    shape, pads = spartan_shape(curve, "dup_empty")
    shape = _extreme_coefficients(shape)
    p, n = shape["p"], max(pads)
    inst = _extreme_instance(shape, kind)
    gens, gens_s = gens_of(curve, n)
    ch = Challenger(p, curve)
    pf = prove_ref(shape, inst, pads[0], pads[1], ch, strict=False)
    i1, i2 = opening_instances(curve, shape, inst, pf, gens)
    ref = open_ref(curve, gens, gens_s, i1, i2, ch)
    with key_of_kind(curve, gens, "pre") as key:
        for is_mont in (False, True):
            with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
                upload_shape(nf, shape, is_mont)
                set_running(nf, inst, p, is_mont)
                prove(nf, pads[0], pads[1], Challenger(p, curve), p, is_mont=is_mont)
                run_opening(nf, key, ref, curve, p, is_mont)


# ------------------------------------------------------------------------------------------------------------- Hyrax ----

@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_hyrax_extremes(gpu_lib, curve, kind):
    """Field-element documents at the extremes, the point at M - 1 / table max, row blinds and per-round blinds at M - 1: every
    call against hyrax_ref, both input forms."""
    from gpu_drivers import hyrax_points, key_of_kind, row_comms, run_hyrax
    from oracle.hyrax_oracle import hyrax_ref
    from oracle.ipa_oracle import compress, gens_of
    from oracle.r1cs_oracle import field
    from oracle.spartan_oracle import Challenger
    from reef_amd._fe import _arr
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    num_vars, left = 7, 3
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    ints = values(kind, p, (1 << num_vars) - 3)
    point = [p - 1 if i % 2 else table_max(p) for i in range(num_vars)]
    row_blinds = values(kind, p, 1 << left)
    blinds = [(p - 1, table_max(p) if k % 2 else 0) for k in range(right)]
    rc = row_comms(curve, gens, ints, num_vars, left, row_blinds, h)
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, num_vars), p, row_blinds=row_blinds, h=h, blinds=blinds,
                    row_comms=rc)
    R = (1 << 256) % p
    with key_of_kind(curve, gens, "pre") as key:
        for is_mont in (False, True):
            z = _arr([v * R % p for v in ints] if is_mont else ints)
            rb = [v * R % p for v in row_blinds] if is_mont else row_blinds
            with HyraxEval(curve, z, num_vars, left, row_blinds=rb, is_mont=is_mont) as hx:
                run_hyrax(hx, key, ref, curve, point, q, is_mont=is_mont, h=h, blinds=blinds)
                assert compress(curve, hx.eval_comm(rc)) == compress(curve, ref["comm_lz"]), "comm_LZ"


def test_values_are_the_extremes():
    """table max really is the element whose internal form is 2^254 - 1 (limbs 0..7 at 2^29 - 1, top limb 2^22 - 1)."""
    for mod in (P, Q):
        t = table_max(mod) * (1 << 261) % mod
        assert t == (1 << 254) - 1
        assert [(t >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] == [(1 << 29) - 1] * 8 and t >> 232 == (1 << 22) - 1
