"""The exceptional cases of the group law through the accumulation kernels themselves, whatever order the sort hands them in.

k_accum0, its merge levels and the bucket reductions call xyzz_madd_flags / xyzz_add_coop on the entries of a bucket in the
order the scatter's atomics left them, so a test cannot place P + P at a chosen step.  Here every order meets it: every base is
one of G, -G, 2G, -2G and the identity, and the scalars are full-width values drawn from a pool of 8, so that a window has at
most 8 live buckets, each with hundreds of entries whose running sum keeps passing through O, +/-G and +/-2G -- doublings,
cancellations, identity entries and accumulators that are the identity in the ZZ = 0 (mod M) form -- and whose chunk sums meet
equal, opposite or empty in the merge and reduce kernels.  Expected value: (sum s_i m_i) G from Python integers, which no
order changes; at 4096 points also the C oracle.  Shapes: the four k_accum0 instantiations over the loop-form tables that
tests/test_gpu_limb_tables.py documents, and a plain key, which reads the packed tables."""
import numpy as np
import pytest

from oracle.pasta_oracle import CURVES, SplitMix64, uniform_scalar

pytestmark = pytest.mark.gpu
CID = {"pallas": 0, "vesta": 1}
MULTIPLES = [1, -1, 2, -2, 0]


def problem(name, n, seed):
    """-> (bases (n, 8) uint64, multiples m_i, scalar pool, pool index r_i)."""
    C = CURVES[name]
    rows = np.stack([np.frombuffer(C.affine_to_bytes(C.mul(k % C.order, C.gen) if k else None), dtype=np.uint64) for k in MULTIPLES])
    rng = np.random.default_rng(seed)
    which = rng.integers(0, len(MULTIPLES), n)
    which[:10] = np.tile(np.arange(5), 2)                 # every base is there, whatever the draw
    sm = SplitMix64(seed)
    pool = [uniform_scalar(sm, C.order) for _ in range(8)]
    return rows[which], np.array(MULTIPLES)[which], pool, rng.integers(0, 8, n)


def scalars(name, pool, r, mont):
    C = CURVES[name]
    vals = [C.scalar_to_mont(v) if mont else v for v in pool]
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)[r]


def expected(name, mult, pool, r, upto):
    C = CURVES[name]
    acc = sum(pool[j] * int(mult[:upto][r[:upto] == j].sum()) for j in range(8))
    return C.compress(C.mul(acc % C.order, C.gen))


def run(name, ctx, n, seed_key, cref=None):
    from reef_amd import msm
    bases, mult, pool, r = seed_key
    for mont in (True, False):
        sc = scalars(name, pool, r, mont)
        for upto in (n, n - 1237):                        # the whole key and a ragged prefix (the last chunk is short)
            got = msm.compress(name, ctx.msm(np.ascontiguousarray(sc[:upto]), is_mont=mont))
            assert got == expected(name, mult, pool, r, upto), (mont, upto)
            if cref is not None:
                oracle = cref.msm_pippenger(CID[name], np.ascontiguousarray(bases[:upto]), np.ascontiguousarray(sc[:upto]), mont=mont, threads=8)
                assert got == cref.compress(CID[name], oracle), (mont, upto)


@pytest.fixture(scope="module")
def small():
    return {name: problem(name, 4096, 0xE5C + CID[name]) for name in CID}


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_4096_points_loop_form(name, chunk, gpu_lib, cref, small):
    from reef_amd import msm
    with msm.MsmContext(name, small[name][0], bucket_groups=1, chunk=chunk) as ctx:
        assert ctx.plan()["tables"] > 1 and not ctx.has_byte_tables()
        run(name, ctx, 4096, small[name], cref)


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_4096_points_plain_key_packed_form(name, gpu_lib, cref, small):
    from reef_amd import msm
    with msm.MsmContext(name, small[name][0], bucket_groups=0) as ctx:
        assert ctx.plan()["tables"] == 1                  # no pre-shifted tables: k_accum0 reads the packed key
        run(name, ctx, 4096, small[name], cref)


@pytest.mark.parametrize("chunk", [0, 8])
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_65536_points_window_15_one_word_entries(name, chunk, gpu_lib):
    from reef_amd import msm
    n = 1 << 16
    key = problem(name, n, 0x1E5C + CID[name])
    with msm.MsmContext(name, key[0], bucket_groups=1, window_bits=15, chunk=chunk) as ctx:
        assert ctx.plan() == {"window_bits": 15, "windows": 18, "bucket_groups": 1, "tables": 18}
        run(name, ctx, n, key)
