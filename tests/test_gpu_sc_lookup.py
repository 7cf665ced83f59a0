"""reef_sc_lookup: entries of the sum-check table (row N2) AS LAST SET, by index -- the v_i = T[q_i] of a step's lookups
(r1cs.rs:2066-2077) once the document's symbols live on the device only.  The oracle is a Python model of the parts written in this
file; every value is a canonical integer mod q, so every comparison is bit-exact.  ell = 12 throughout: 4096 entries, 16 blocks."""
import numpy as np
import pytest

from oracle.pasta_oracle import SplitMix64, uniform_scalar
from oracle.sumcheck_oracle import Q, gen_eq_table, linear_mle_coeffs, linear_mle_fold

pytestmark = pytest.mark.gpu

ELL = 12
N = 1 << ELL
N_FE, N_FILL, N_SYM = 37, 91, 1000            # part boundaries at 37, 128 and 1128; zero from 1128 on
# 0, both sides of every part boundary, the last entry, a repeated index (36 and 1127 again)
EDGES = [0, 36, 37, 127, 128, 1127, 1128, N - 1, 36, 1127]
SIZES = [0, 1, 64, 65, 257]                   # below, at and across a wave and a 256-lane block


def _model(parts):
    """The table the parts describe as a list of N ints: the parts laid end to end from entry 0, zero beyond them."""
    t = []
    for part in parts:
        if part[0] == "fill":
            t += [int(part[1])] * part[2]
        else:
            t += [int(v) for v in part[1]]
    assert len(t) <= N
    return t + [0] * (N - len(t))


def _parts(dtype, seed):
    """[FE 37, FILL x 91, SYMBOLS dtype x 1000] with symbols over the whole range of the type, its maximum at both ends of the run."""
    rng = SplitMix64(seed)
    top = int(np.iinfo(dtype).max)
    sym = np.array([rng.next() % (top + 1) for _ in range(N_SYM)], dtype=dtype)
    sym[0] = sym[-1] = sym[N_SYM // 2] = top
    return [("fe", [uniform_scalar(rng, Q) for _ in range(N_FE)]), ("fill", uniform_scalar(rng, Q), N_FILL), ("symbols", sym)]


def _tables():
    rng = SplitMix64(1201)
    ints = [uniform_scalar(rng, Q) for _ in range(N - 5)]          # set_table pads the last five with zero
    ints[0], ints[1] = Q - 1, 0
    yield "ints", ("ints", ints), ints + [0] * 5
    for dtype in (np.uint8, np.uint16, np.uint32):
        parts = _parts(dtype, 1200 + np.dtype(dtype).itemsize)
        yield "parts-" + np.dtype(dtype).name, ("parts", parts), _model(parts)


TABLES = {name: (how, model) for name, how, model in _tables()}


def _set(sc, how):
    if how[0] == "ints":
        sc.set_table(0, how[1])
    else:
        sc.set_table_parts(how[1])


def _indices(k, seed):
    """k indices: the edges first (as many as fit), seeded ones after them."""
    rng = SplitMix64(seed)
    return (EDGES + [rng.next() % N for _ in range(max(0, k - len(EDGES)))])[:k]


@pytest.mark.parametrize("name", list(TABLES))
def test_lookup_values_host_and_device(name, gpu_lib):
    """Every table form, every size, both destinations.  The 257-index call carries all the edges; the edges alone are asked once more
    so that the 1-, 64- and 65-index calls' truncation of them cannot hide one."""
    from reef_amd.msm import DeviceBuffer
    from reef_amd.sumcheck import SumCheck, array_to_ints
    how, model = TABLES[name]
    with SumCheck("pallas", ELL) as sc:
        _set(sc, how)
        assert sc.lookup(EDGES) == [model[i] for i in EDGES]
        for k in SIZES:
            idx = _indices(k, 7 * k + 1)
            want = [model[i] for i in idx]
            assert sc.lookup(idx) == want, (name, k)
            sentinel = np.full((k + 1, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            dbuf = DeviceBuffer.from_host(sentinel)
            sc.lookup(idx, out=dbuf)
            got = dbuf.to_host((k + 1, 4))
            assert array_to_ints(got[:k]) == want, (name, k, "device")
            assert (got[k] == sentinel[k]).all(), "the call wrote past its k entries"
            dbuf.free()


@pytest.mark.parametrize("name", ["ints", "parts-uint8"])
def test_lookup_does_not_depend_on_the_folds(name, gpu_lib):
    """After 0, 1 and ell folds the answers are those of the table as set, and after a reset as well."""
    from reef_amd.sumcheck import SumCheck
    how, model = TABLES[name]
    rng = SplitMix64(77)
    idx = _indices(65, 5)
    want = [model[i] for i in idx]
    rs = [uniform_scalar(rng, Q) for _ in range(4)]
    last_q = [uniform_scalar(rng, Q) for _ in range(ELL)]
    with SumCheck("pallas", ELL) as sc:
        _set(sc, how)
        sc.gen_eq_table(rs, [0, 1127, N - 1], last_q)
        assert sc.lookup(idx) == want
        for i in range(1, ELL + 1):
            sc.fold(i, uniform_scalar(rng, Q))
            if i in (1, ELL):
                assert sc.lookup(idx) == want, i
        sc.reset_table()
        assert sc.lookup(idx) == want


def _step(sc, t, rs, qs, last_q, challenges, idx, want, fused):
    """One folding step as the prover drives it; idx is not None: a lookup before the first round and after every round."""
    e = gen_eq_table(rs, qs, last_q, Q)
    tt = list(t)
    sc.reset_table()
    sc.gen_eq_table(rs, qs, last_q)
    seen = []
    if idx is not None:
        assert sc.lookup(idx) == want
    g = sc.round_coeffs(1)
    for i in range(1, ELL + 1):
        seen.append(g)
        assert g == linear_mle_coeffs(tt, e, ELL, i, Q), i
        linear_mle_fold(tt, e, ELL, i, challenges[i - 1], Q)
        if fused and i < ELL:
            g = sc.fold_and_next_coeffs(i, challenges[i - 1])
            if idx is not None:
                assert sc.lookup(idx) == want, i
        else:
            sc.fold(i, challenges[i - 1])
            if idx is not None:
                assert sc.lookup(idx) == want, i
            if i < ELL:
                g = sc.round_coeffs(i + 1)
    seen.append(sc.read(0, 1))
    assert seen[-1] == [tt[0]]
    return seen


@pytest.mark.parametrize("forced", [False, True], ids=["shipped", "structured-forced"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-call"])
def test_rounds_are_the_same_with_lookups_between_them(fused, forced, gpu_lib, either_build_for, monkeypatch):
    """A step's coefficients and final value with a lookup between every two rounds equal the same step's without, and the oracle's.
    forced: the experiment build with the rank-one / structured rounds switched on at this size, where a lookup that wrote the
    deferred fold out, or marked the table as folded, would change which kernels the next round runs."""
    from reef_amd.sumcheck import SumCheck
    either_build_for(forced)
    if forced:
        monkeypatch.setenv("REEF_SC_RANK1_MIN_POW", "1")
    how, model = TABLES["parts-uint8"]
    rng = SplitMix64(99)
    qs = [0, 36, 37, 1127, N - 1, 36]
    rs = [uniform_scalar(rng, Q) for _ in range(len(qs) + 1)]
    last_q = [uniform_scalar(rng, Q) for _ in range(ELL)]
    challenges = [uniform_scalar(rng, Q) for _ in range(ELL)]
    idx = _indices(65, 3)
    want = [model[i] for i in idx]
    with SumCheck("pallas", ELL) as sc:
        _set(sc, how)
        without = _step(sc, model, rs, qs, last_q, challenges, None, None, fused)
        with_lookups = _step(sc, model, rs, qs, last_q, challenges, idx, want, fused)
        assert with_lookups == without


@pytest.fixture
def either_build_for(monkeypatch):
    """-> a function: (True) bind the experiment build for the rest of the test, as conftest's experiment_build does."""
    def pick(experiment):
        if experiment:
            from reef_amd import _ffi
            exp = _ffi.load_experiment()
            assert not _ffi.is_release(exp)
            monkeypatch.setattr(_ffi, "_lib", exp)
    return pick


def test_an_index_past_the_table_is_refused_and_nothing_is_written(gpu_lib):
    from reef_amd import _ffi
    from reef_amd.msm import DeviceBuffer
    from reef_amd.sumcheck import SumCheck
    how, _ = TABLES["parts-uint16"]
    with SumCheck("pallas", ELL) as sc:
        _set(sc, how)
        idx = np.array([0, 5, N, 7, N + 3], dtype=np.uint64)
        host = np.full((len(idx), 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        before = host.copy()
        st = gpu_lib.reef_sc_lookup(sc._h, idx.ctypes.data, len(idx), host.ctypes.data, _ffi.REEF_HOST)
        msg = gpu_lib.reef_last_error().decode()
        assert st == 1, st                                         # REEF_ERR_ARG
        assert "idx[2]" in msg and str(N) in msg, msg                  # the FIRST offending index, by position and value
        assert (host == before).all()
        dbuf = DeviceBuffer.from_host(before)
        assert gpu_lib.reef_sc_lookup(sc._h, idx.ctypes.data, len(idx), dbuf.ptr, _ffi.REEF_DEVICE) == 1
        assert (dbuf.to_host(before.shape) == before).all()
        with pytest.raises(_ffi.ReefError) as err:
            sc.lookup([N])
        assert err.value.status == 1
        assert sc.lookup([N - 1, 0]) == [0, int(how[1][0][1][0])]     # the ctx is as usable as before


def test_a_ctx_without_a_table_is_refused(gpu_lib):
    from reef_amd import _ffi
    from reef_amd.sumcheck import SumCheck
    rng = SplitMix64(5)
    with SumCheck("pallas", ELL) as sc:
        with pytest.raises(_ffi.ReefError) as err:
            sc.lookup([0])
        assert err.value.status == 1 and "no table" in str(err.value)
        assert sc.lookup([]) == []                                   # k = 0 is REEF_OK whatever the ctx holds
        sc.set_table(1, [uniform_scalar(rng, Q) for _ in range(8)])  # an EQ table is not a table to look up in
        with pytest.raises(_ffi.ReefError):
            sc.lookup([0])
        sc.set_table(0, [3, 4])
        assert sc.lookup([1, 0, 2]) == [4, 3, 0]
