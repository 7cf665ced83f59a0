"""The deep fold on the GPU (include/reef_msm.h: reef_fold_deep, reef_msm_ctx_create_folded) and the nibble route of the IPA cross terms.

reef_fold_deep gives the generators k folds away from a resident key in one pass; it is compared, as affine points and bit for bit, with
k successive reef_fold calls and with the big-integer oracle's MSM over the cosets points[j::n_k] with the coefficient vector
s_t = prod_m (bit_{k-1-m}(t) ? w2[m] : w1[m]).  Shapes: n = 2^3 .. 2^10 with k in {0, 1, 2, 3, log2 n - 1, log2 n} on a plain and a
nibble-table key (n_k = 64 and 128, a full wave and two, are among them; n = 1024 with k = 10 is one output of 1024 terms), n = 2^13 with
k = 3 on a pre-shifted key (the Hyrax case: 1024 outputs of 8 terms), n = 2048 with byte tables.  Scalars: random, 0, 1, r - 1, w1 = w2;
the 255-bit form (no coefficient is known for which glv_split fails, tests/test_host_math.py has none: the +experiment build's switch
REEF_FOLD_DEEP_GLV=0 sends every coefficient down that form).  Generators at the group law's corners: G_{i+half} = G_i (a bucket adds
P + P), G_{i+half} = -G_i with w1 = w2 (the identity, back as (0, 0)), identity points in the key.  Then the folded points as a resident
key (n_k = 1, 16, 1024, 2048) against reef_msm_folded over the source, reef_ipa_cross_terms on small pre-shifted keys against a plain key
of the same points, and the argument errors, each with nothing written."""
import random

import numpy as np
import pytest

from oracle import pasta_ref
from oracle.ipa_oracle import affine, msm as ref_msm
from oracle.r1cs_oracle import field
from reef_amd._fe import _arr

pytestmark = pytest.mark.gpu

BASE_MODULUS = {0: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,     # Pallas: coordinates in Fp
                1: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001}     # Vesta: coordinates in Fq

_GENS = {}


def _gens(curve, n):
    if (curve, n) not in _GENS:
        _GENS[(curve, n)] = pasta_ref.gen_bases_ap(curve, 11, 3, n)
    return _GENS[(curve, n)]


def _coefs(w1s, w2s, p):
    k = len(w1s)
    out = []
    for t in range(1 << k):
        s = 1
        for m in range(k):
            s = s * (w2s[m] if (t >> (k - 1 - m)) & 1 else w1s[m]) % p
        out.append(s)
    return out


def _oracle_fold(curve, gens, w1s, w2s):
    """G^(k)_j as the oracle's MSM over the coset gens[j::n_k], affine"""
    p = field(curve)
    n_k = gens.shape[0] >> len(w1s)
    s = _coefs(w1s, w2s, p)
    return np.stack([affine(curve, ref_msm(curve, gens[j::n_k], s)) for j in range(n_k)])


def _successive_folds(curve, gens, w1s, w2s):
    from reef_amd import msm
    for w1, w2 in zip(w1s, w2s):
        gens = msm.fold(curve, np.ascontiguousarray(gens), gens.shape[0] // 2, w1, w2)
    return gens


def _key(curve, gens, kind):
    from reef_amd.msm import MsmContext
    kw = {"plain": {}, "pre": dict(bucket_groups=1), "nibble": dict(bucket_groups=1), "tables": dict(bucket_groups=1, byte_tables=1)}[kind]
    key = MsmContext(curve, np.ascontiguousarray(gens), **kw)
    assert key.has_byte_tables() == (kind == "tables")
    return key


def _challenges(curve, k, seed):
    p = field(curve)
    rng = random.Random(seed)
    return [rng.randrange(p) for _ in range(k)], [rng.randrange(p) for _ in range(k)]


def _check(curve, gens, w1s, w2s, kinds, oracle=True):
    from reef_amd import msm
    want = _successive_folds(curve, gens, w1s, w2s)
    if oracle:
        assert np.array_equal(want, _oracle_fold(curve, gens, w1s, w2s)), "k folds against the oracle"
    for kind in kinds:
        with _key(curve, gens, kind) as key:
            got = msm.fold_deep(key, w1s, w2s)
            assert got.shape == want.shape
            assert np.array_equal(got, want), f"{kind} key, n = {gens.shape[0]}, k = {len(w1s)}"
    return want


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logn", range(3, 11))
def test_parity_with_k_folds_and_the_oracle(gpu_lib, curve, logn):
    n = 1 << logn
    gens = _gens(curve, n)
    for k in sorted({0, 1, 2, 3, logn - 1, logn}):
        w1s, w2s = _challenges(curve, k, 100 * logn + k)
        _check(curve, gens, w1s, w2s, ("plain", "nibble"))


@pytest.mark.parametrize("curve", [0, 1])
def test_the_hyrax_case_on_a_pre_shifted_key(gpu_lib, curve):
    """n = 2^13, k = 3: 1024 outputs of 8 terms"""
    w1s, w2s = _challenges(curve, 3, 13)
    _check(curve, _gens(curve, 1 << 13), w1s, w2s, ("pre",))


@pytest.mark.parametrize("curve", [0, 1])
def test_a_byte_table_key(gpu_lib, curve):
    gens = _gens(curve, 2048)
    for k in (1, 4, 11):
        w1s, w2s = _challenges(curve, k, 2048 + k)
        _check(curve, gens, w1s, w2s, ("tables",), oracle=k != 1)     # k = 1: 1024 oracle MSMs of two terms say nothing k = 4 does not


@pytest.mark.parametrize("curve", [0, 1])
def test_special_scalars(gpu_lib, curve):
    p = field(curve)
    gens = _gens(curve, 64)
    rng = random.Random(5 + curve)
    x = rng.randrange(p)
    for w1s, w2s in (([0, 1, p - 1], [1, p - 1, 0]),            # coefficients 0, +-1
                     ([0, 0], [0, 0]),                           # every coefficient zero: every output the identity
                     ([1, 1, 1], [1, 1, 1]),                     # the plain sum of each coset
                     ([x, 5, p - 1], [x, 5, p - 1]),             # w1 = w2
                     ([p - 1] * 6, [x] + [p - 1] * 5)):          # down to one point
        want = _check(curve, gens, w1s, w2s, ("plain", "nibble"))
        if not any(w1s + w2s):
            assert not want.any(), "the identity is (0, 0)"


@pytest.mark.parametrize("curve", [0, 1])
def test_the_255_bit_form(experiment_build, gpu_lib, curve, monkeypatch):
    """REEF_FOLD_DEEP_GLV=0 (+experiment build only): the coefficients are not split, one half of up to 86 windows."""
    monkeypatch.setenv("REEF_FOLD_DEEP_GLV", "0")
    gens = _gens(curve, 128)
    p = field(curve)
    for k, seed in ((1, 1), (3, 2), (7, 3)):
        w1s, w2s = _challenges(curve, k, 255 + seed)
        _check(curve, gens, w1s, w2s, ("plain", "nibble"))
    _check(curve, gens, [p - 1, 0], [1, p - 1], ("plain",))


def _neg(curve, pts):
    """-P for ABI affine points (Montgomery coordinates: -y is modulus - y there too); (0, 0) stays"""
    q = BASE_MODULUS[curve]
    out = pts.copy()
    for i in range(pts.shape[0]):
        y = pasta_ref.limbs_to_int(pts[i, 4:])
        if pts[i].any():
            out[i, 4:] = pasta_ref.int_to_limbs((q - y) % q)
    return out


@pytest.mark.parametrize("curve", [0, 1])
def test_generators_at_the_corners_of_the_group_law(gpu_lib, curve):
    p = field(curve)
    base = _gens(curve, 64)
    rng = random.Random(77 + curve)
    x = rng.randrange(p)
    # G_{i+half} = G_i: with equal digits a bucket adds P + P
    same = np.vstack([base[:32], base[:32]])
    _check(curve, same, [x], [x], ("plain", "nibble"))
    _check(curve, same, [3, x], [3, 7], ("plain",))
    # G_{i+half} = -G_i with w1 = w2: every output is the identity, (0, 0)
    opposite = np.vstack([base[:32], _neg(curve, base[:32])])
    assert not _check(curve, opposite, [x], [x], ("plain", "nibble")).any()
    # identity points in the key: alone in a coset, with a partner, and a whole coset of them
    holes = base.copy()
    holes[[0, 5, 37, 40, 8, 24, 56]] = 0
    for k in (0, 1, 2, 6):
        w1s, w2s = _challenges(curve, k, 900 + k)
        _check(curve, holes, w1s, w2s, ("plain", "nibble"))


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n,k", [(64, 6), (128, 3), (4096, 2), (4096, 1)])       # n_k = 1, 16, 1024, 2048
def test_the_folded_points_as_a_resident_key(gpu_lib, curve, n, k):
    from reef_amd import msm
    p = field(curve)
    gens = _gens(curve, n)
    w1s, w2s = _challenges(curve, k, n + k)
    rng = random.Random(n * k)
    n_k = n >> k
    v = _arr([rng.randrange(p) for _ in range(n_k)])
    with _key(curve, gens, "pre" if n > 1024 else "nibble") as src, src.folded(w1s, w2s) as key:
        assert key.n == n_k and key.plan()["bucket_groups"] == 1
        got = msm.compress(curve, key.msm(v, is_mont=False))
        assert got == msm.compress(curve, src.msm_folded(v, w1s, w2s, is_mont=False))
        assert np.array_equal(msm.fold_deep(key, [], []), msm.fold_deep(src, w1s, w2s)), "k = 0 copies the key: the folded points"
    with _key(curve, gens, "plain") as src, src.folded(w1s, w2s, bucket_groups=0) as key:       # a plain source, a plain folded key
        assert msm.compress(curve, key.msm(v, is_mont=False)) == got


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [16, 1024])
def test_cross_terms_on_a_nibble_table_key(gpu_lib, curve, n):
    """reef_ipa_cross_terms on a small pre-shifted key goes through its nibble tables: the same L and R as on a plain key"""
    from reef_amd import msm
    p = field(curve)
    gens = _gens(curve, n)
    logn = n.bit_length() - 1
    rng = random.Random(n + curve)
    with _key(curve, gens, "nibble") as small, _key(curve, gens, "plain") as plain:
        for k in (0, 2, logn - 1):
            w1s, w2s = _challenges(curve, k, 31 * n + k)
            a = _arr([rng.randrange(p) for _ in range(n >> k)])
            for is_mont in (False, True):
                got = small.ipa_cross_terms(a, w1s, w2s, is_mont=is_mont)
                want = plain.ipa_cross_terms(a, w1s, w2s, is_mont=is_mont)
                assert [msm.compress(curve, x) for x in got] == [msm.compress(curve, x) for x in want], (k, is_mont)
        zero = small.ipa_cross_terms(_arr([0] * n), [], [], is_mont=False)
        assert [msm.compress(curve, x) for x in zero] == [bytes(32)] * 2


@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors_write_nothing(gpu_lib, curve):
    from reef_amd import msm
    from reef_amd.msm import MsmContext, ReefError
    p = field(curve)
    gens = _gens(curve, 64)[:24]
    mark = np.full((24, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)

    def refused(key, w1s, w2s):
        out = mark.copy()
        with pytest.raises(ReefError) as e:
            msm.fold_deep(key, w1s, w2s, out)
        assert e.value.status == 1 and np.array_equal(out, mark)
        with pytest.raises(ReefError) as e:
            key.folded(w1s, w2s)
        assert e.value.status == 1

    with MsmContext(curve, np.ascontiguousarray(gens)) as key:                    # 24 = 8 * 3 points
        assert msm.fold_deep(key, [2, 3, 4], [5, 6, 7]).shape == (3, 8)           # a multiple of 2^3: legal
        refused(key, [2] * 4, [3] * 4)                                           # not a multiple of 2^4
        refused(key, [2] * 32, [3] * 32)                                         # k > 31
        refused(key, [1, p], [1, 1])                                             # a scalar that is not below the modulus
        refused(key, [1, 1], [(1 << 256) - 1, 1])
        key.set_window_split(1, 2)
        refused(key, [2], [3])                                                   # a ctx with a window split
