"""A pre-shifted key that the bucket pipeline serves keeps a second copy of its tables in the accumulation loop's own form
(engine.inc: Key::limb_tables, ec.h: affine_limbs) and k_accum0 reads its operands from there.  Everything here is checked against
the C oracle or the discrete-logarithm closed form on arithmetic-progression bases, as compressed encodings, on both curves and for
scalars in both conventions.  Which k_accum0 a shape reaches (msm_plan.h: core_launch_plan, merge_plan): the first merge level is fused into
it between 385 and 1024 waves of chunks, entries are one word each from 2^20 entries on; `chunk` (entries per thread) moves a shape of
a given size from one side to the other, so every instantiation over the loop-form tables is reached at sizes the oracle can handle:
    4096 points, 20 tables, default chunk   320 waves    two-word entries
    4096 points, 20 tables, chunk = 2       640 waves    two-word entries, fused
    2^16 points, 18 tables, default chunk   1024 waves   one-word entries, fused
    2^16 points, 18 tables, chunk = 8       2304 waves   one-word entries: the instantiation a 2^20-point MSM runs"""
import numpy as np
import pytest

from oracle.pasta_oracle import CURVES, SplitMix64, uniform_scalar

pytestmark = pytest.mark.gpu
CID = {"pallas": 0, "vesta": 1}
N = 4096


def limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def as_array(ints):
    return np.array([limbs(v) for v in ints], dtype=np.uint64).reshape(len(ints), 4)


def both_conventions(name, ints):
    """-> [(is_mont, scalars)] for the same canonical values."""
    C = CURVES[name]
    return [(False, as_array(ints)), (True, as_array([C.scalar_to_mont(v) for v in ints]))]


@pytest.fixture(scope="module")
def keys(cref):
    """Per curve: 4096 bases in arithmetic progression (the oracle's generator), unchanged by the tests."""
    return {name: cref.gen_bases_ap(CID[name], 0x11AB + CID[name], 13, N) for name in CID}


def want(cref, name, bases, sc, mont):
    return cref.compress(CID[name], cref.msm_pippenger(CID[name], bases, sc, mont=mont, threads=8))


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_4096_points_default_window(name, chunk, gpu_lib, cref, keys):
    from reef_amd import msm
    cid, bases = CID[name], keys[name]
    with msm.MsmContext(name, bases, bucket_groups=1, chunk=chunk) as ctx:
        assert ctx.plan()["tables"] > 1 and not ctx.has_byte_tables()
        for mont in (True, False):
            for kind in (0, 1):                                                  # uniform and witness-like
                sc = cref.gen_scalars(cid, 40 + kind, N, kind=kind, mont=mont)
                assert msm.compress(name, ctx.msm(sc, is_mont=mont)) == want(cref, name, bases, sc, mont), (mont, kind)


@pytest.mark.parametrize("chunk", [0, 8])
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_65536_points_window_15_one_word_entries(name, chunk, gpu_lib):
    """2^16 points at window_bits = 15: 18 tables (signed digits: 18 windows), 2^14 buckets, 18 * 2^16 >= 2^20 entries -- the two-level sort with one-word entries.
    Expected value: the discrete-log closed form; also a ragged prefix (the last chunk is short)."""
    from reef_amd import msm
    C = CURVES[name]
    n, k0, d = 1 << 16, 0x2345671, 0x3B5
    bases = msm.gen_bases(name, k0, d, n, device=True)
    idx = np.arange(n, dtype=object)
    with msm.MsmContext(name, bases, n, bucket_groups=1, window_bits=15, chunk=chunk) as ctx:
        assert ctx.plan() == {"window_bits": 15, "windows": 18, "bucket_groups": 1, "tables": 18}
        for mont in (True, False):
            sc_dev = msm.gen_scalars(name, 0xFACE + mont, n, kind=0, mont=mont, device=True)
            canon = msm.gen_scalars(name, 0xFACE + mont, n, kind=0, mont=False)
            cols = [canon[:, j].astype(object) for j in range(4)]
            for upto in (n, n - 4321):
                acc = 0
                for j in range(4):
                    acc += (int(np.sum(cols[j][:upto])) * k0 + int(np.sum(cols[j][:upto] * idx[:upto])) * d) << (64 * j)
                got = msm.compress(name, ctx.msm(sc_dev, upto, is_mont=mont))
                assert got == C.compress(C.mul(acc % C.order, C.gen)), (mont, upto)


def all_negative_digits(c, n, seed):
    """Scalars whose c-bit windows all lie in 2^(c-1) + 1 .. 2^c - 2: with or without a carry from below every one of them recodes to
    a negative digit and carries on.  (The carry out of the last of them is a digit +1 -- a positive scalar has a positive top digit.)"""
    rng = SplitMix64(seed)
    half = 1 << (c - 1)
    used = 250 // c
    return [sum((half + 1 + rng.next() % (half - 2)) << (c * w) for w in range(used)) for _ in range(n)]


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_degenerate_keys_and_scalars(name, gpu_lib, cref, keys):
    from reef_amd import msm
    cid, C = CID[name], CURVES[name]
    bases = keys[name].copy()
    bases[0] = 0                                                                     # identity points in the key: first, last, inside
    bases[N - 1] = 0
    bases[N // 3] = 0
    bases[101] = bases[100]                                                          # the same point twice
    neg = C.neg(C.affine_from_bytes(bases[200].tobytes()))
    bases[201] = np.frombuffer(C.affine_to_bytes(neg), dtype=np.uint64)              # P and -P
    rng = SplitMix64(77 + cid)
    order = C.order
    with msm.MsmContext(name, bases, bucket_groups=1) as ctx:
        c = ctx.plan()["window_bits"]
        uniform = [uniform_scalar(rng, order) for _ in range(N)]
        pairs = list(uniform)
        pairs[101] = pairs[100]                                                      # equal scalars: the doubling branch in every bucket they meet in
        pairs[201] = pairs[200]                                                      # equal scalars on P and -P: they cancel in every bucket
        cases = {
            "identity points, doubling, cancellation": pairs,
            "all scalars equal": [uniform[7]] * N,                                   # one bucket per window, and the pairs above meet in it
            "negative digits": all_negative_digits(c, N, 5 + cid),
            "zero scalars": [0] * N,
            "zero but one": [0] * (N - 1) + [uniform[3]],
            "minus one": [order - 1] * N,
        }
        for label, ints in cases.items():
            for mont, sc in both_conventions(name, ints):
                got = msm.compress(name, ctx.msm(sc, is_mont=mont))
                assert got == want(cref, name, bases, sc, mont), (label, mont)
        assert msm.compress(name, ctx.msm(as_array([0] * N), is_mont=False)) == bytes(32)


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_paths_that_share_the_key(name, gpu_lib, cref, keys):
    """A clone, a window split over two clones, msm_rows with rows shorter than the key, and a context whose bases are replaced --
    by a longer key, so that its tables are allocated again -- and then used."""
    from reef_amd import msm
    cid, bases = CID[name], keys[name]
    for mont in (True, False):
        sc = cref.gen_scalars(cid, 91, N, mont=mont)
        exp = want(cref, name, bases, sc, mont)
        with msm.MsmContext(name, bases, bucket_groups=1) as ctx:
            assert msm.compress(name, ctx.msm(sc, is_mont=mont)) == exp
            with ctx.clone() as a, ctx.clone() as b:
                assert msm.compress(name, a.msm(sc, is_mont=mont)) == exp
                a.set_window_split(0, 2)
                b.set_window_split(1, 2)
                parts = np.stack([a.msm(sc, is_mont=mont), b.msm(sc, is_mont=mont)])
                assert msm.compress(name, parts[0]) != exp                           # a partial sum, not the total
                assert msm.compress(name, msm.sum_points(name, parts)) == exp
            rows, row_len = 3, 1500                                                  # rows shorter than the key
            rsc = cref.gen_scalars(cid, 92, rows * row_len, mont=mont)
            exp_rows = cref.compress(cid, cref.row_msm(cid, bases[:row_len], rsc, rows, row_len, mont=mont, threads=8))
            assert msm.compress(name, ctx.msm_rows(rsc, rows, row_len, is_mont=mont)) == exp_rows
            assert msm.compress(name, ctx.msm(sc, is_mont=mont)) == exp              # the key is what it was
            for n2, seed in ((6000, 93), (2048, 94)):                                # other bases: longer (new tables), then shorter (the same buffers)
                other = cref.gen_bases_ap(cid, 0x77 + seed, 5, n2)
                sc2 = cref.gen_scalars(cid, seed, n2, mont=mont)
                ctx.set_bases(other)
                assert msm.compress(name, ctx.msm(sc2, is_mont=mont)) == want(cref, name, other, sc2, mont), n2


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_forced_packed_form_gives_the_same_encodings(name, gpu_lib, cref, keys, experiment_build, monkeypatch):
    """REEF_MSM_LIMB_TABLES=0 (experiment build; read when a key is built) keeps the key in the packed tables alone: the same
    encodings as the default, and the oracle's."""
    from reef_amd import msm
    cid, bases = CID[name], keys[name]
    got = {}
    for form in ("default", "0"):
        if form == "0":
            monkeypatch.setenv("REEF_MSM_LIMB_TABLES", "0")
        else:
            monkeypatch.delenv("REEF_MSM_LIMB_TABLES", raising=False)
        with msm.MsmContext(name, bases, bucket_groups=1) as ctx, msm.MsmContext(name, bases, bucket_groups=1, chunk=2) as fused:
            got[form] = []
            for mont in (True, False):
                for kind in (0, 1):
                    sc = cref.gen_scalars(cid, 60 + kind, N, kind=kind, mont=mont)
                    enc = msm.compress(name, ctx.msm(sc, is_mont=mont))
                    assert enc == msm.compress(name, fused.msm(sc, is_mont=mont))
                    assert enc == want(cref, name, bases, sc, mont), (form, mont, kind)
                    got[form].append(enc)
    assert got["default"] == got["0"]
