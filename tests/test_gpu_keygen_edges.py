"""Row N1 at its edges: reef_derive_generators against oracle/keygen_oracle.py, bit-exact, where tests/test_gpu_keygen.py does not go.
A  BLAKE2b block edges: domain-separation strings whose messages end on, one before and one after a block boundary, 0 and 255 bytes
B  argument forms: parameters in Montgomery form, output left on the device, labels across the SHAKE rate
C  the engine's pieces: n = PIECE - 1, PIECE, PIECE + 1, 2 PIECE, 2 PIECE + 1 -- prefixes of one another, the oracle at every seam
D  the two branches of sswu_iso a hashed u never takes (tv2 = 0; a point of the isogeny's kernel), reached with crafted z and b
E  refused arguments, and the call after a refusal
F  parameters that are not below the modulus are refused
The inputs are tests/keygen_inputs.py; tests/test_keygen_inputs_host.py proves on the CPU that they hit what they claim."""
import ctypes
import functools

import numpy as np
import pytest

import keygen_inputs as I
from oracle import keygen_oracle as K

pytestmark = pytest.mark.gpu

CURVES = ("pallas", "vesta")
REEF_ERR_ARG = 1
R256 = 1 << 256


def _derive(curve, label, n, k, **kw):
    from reef_amd import keygen
    return keygen.derive_generators(curve, label, n, k.a, k.b, k.z, k.iso, k.dst, k.little_endian, **kw)


def _ints(curve, raw):
    from reef_amd import keygen
    return keygen.points_to_ints(curve, raw)


@functools.lru_cache(maxsize=None)
def _oracle_point(curve, label, i):
    """generator i of the label under the stand-in set: the stream is a prefix of itself, so the same for every n > i"""
    return K.hash_to_curve(K.shake256_chunks(label, i + 1)[i], I.standin(curve))


# ---- A: block edges ----

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("dl", I.DST_LENGTHS)
def test_dst_lengths_at_the_block_edges(curve, dl, gpu_lib):
    for le in (False, True) if dl in I.BOTH_ORDERS else (False,):
        k = I.with_params(I.standin(curve, 0, le), dst=I.dst_of(dl))
        assert _ints(curve, _derive(curve, b"ck", 3, k)) == K.from_label(b"ck", 3, k), (dl, le)


@pytest.mark.parametrize("curve", CURVES)
def test_a_dst_of_256_bytes_is_refused(curve, gpu_lib):
    from reef_amd._ffi import ReefError
    with pytest.raises(ReefError) as e:
        _derive(curve, b"ck", 3, I.with_params(I.standin(curve), dst=I.dst_of(256)))
    assert e.value.status == REEF_ERR_ARG


# ---- B: forms ----

@pytest.mark.parametrize("curve", CURVES)
def test_montgomery_form_parameters(curve, gpu_lib):
    k = I.standin(curve)
    canon = _derive(curve, I.REGULAR_LABEL, I.REGULAR_N, k)
    mont = _derive(curve, I.REGULAR_LABEL, I.REGULAR_N, k, is_mont=True)
    assert np.array_equal(canon, mont)
    assert _ints(curve, mont) == K.from_label(I.REGULAR_LABEL, I.REGULAR_N, k)


@pytest.mark.parametrize("curve,n", (("pallas", I.REGULAR_N), ("vesta", I.REGULAR_N), ("pallas", I.PIECE + 1)))
def test_device_output_is_the_host_output(curve, n, gpu_lib):
    k = I.standin(curve)
    host = _derive(curve, I.REGULAR_LABEL, n, k)
    buf = _derive(curve, I.REGULAR_LABEL, n, k, device=True)
    dev = buf.to_host((n, 8))
    buf.free()
    assert host.any() and np.array_equal(host, dev)
    if n == I.REGULAR_N:
        assert _ints(curve, dev) == K.from_label(I.REGULAR_LABEL, n, k)


@pytest.mark.parametrize("curve", CURVES)
def test_labels_across_the_shake_rate(curve, gpu_lib):
    k = I.standin(curve)
    for size in (135, 136, 137, 1000):
        label = bytes((7 * j + size) & 0xFF for j in range(size))
        assert _ints(curve, _derive(curve, label, 2, k)) == K.from_label(label, 2, k), size


# ---- C: pieces ----

PIECE_SIZES = {"pallas": (I.PIECE - 1, I.PIECE, I.PIECE + 1, 2 * I.PIECE), "vesta": (2 * I.PIECE + 1,)}


@pytest.fixture(scope="module")
def largest():
    """the derivation at the largest n of each curve, made on first use and never changed"""
    cache = {}

    def get(curve):
        if curve not in cache:
            cache[curve] = _derive(curve, b"ck", max(PIECE_SIZES[curve]), I.standin(curve))
            cache[curve].setflags(write=False)
        return cache[curve]
    return get


@pytest.mark.parametrize("curve,n", [(c, n) for c in CURVES for n in PIECE_SIZES[c]])
def test_piece_sizes_are_prefixes_and_match_the_oracle_at_the_seams(curve, n, largest, gpu_lib):
    big = largest(curve)
    raw = big if n == len(big) else _derive(curve, b"ck", n, I.standin(curve))
    assert raw.shape == (n, 8) and np.array_equal(raw, big[:n])
    seams = I.seam_indices(n)
    assert _ints(curve, raw[seams]) == [_oracle_point(curve, b"ck", i) for i in seams]


@pytest.mark.parametrize("curve", CURVES)
def test_every_point_of_the_largest_derivation_is_on_the_curve(curve, largest, gpu_lib):
    p = I.standin(curve).p
    pts = _ints(curve, largest(curve))
    assert len(pts) == max(PIECE_SIZES[curve]) and None not in pts
    assert all((y * y - x * x * x - 5) % p == 0 for x, y in pts)
    assert len(np.unique(largest(curve), axis=0)) == len(pts)


# ---- D: branches ----

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("le", (False, True))
@pytest.mark.parametrize("gi,which", I.TV2_TARGETS)
@pytest.mark.parametrize("is_mont", (False, True))
def test_tv2_zero(curve, le, gi, which, is_mont, gpu_lib):
    label, k = I.tv2_zero_case(curve, le, gi, which)
    assert _ints(curve, _derive(curve, label, 2, k, is_mont=is_mont)) == K.from_label(label, 2, k)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("le", (False, True))
@pytest.mark.parametrize("n,gi,which", I.ISO_TARGETS)
def test_a_point_of_the_isogeny_kernel(curve, le, n, gi, which, gpu_lib):
    label, k = I.iso_kernel_case(curve, le, n, gi, which)
    assert _ints(curve, _derive(curve, label, n, k)) == K.from_label(label, n, k)


# ---- E, F: refusals ----

def _struct(k, is_mont=False, **raw):
    """reef_keygen_params of the set k, in the form is_mont says; `raw` elements (a, b, z, or iso as {index: value}) go in as given"""
    from reef_amd import keygen
    form = lambda v: v * R256 % k.p if is_mont else v                              # noqa: E731
    a, b, z = (raw.get(name, form(getattr(k, name))) for name in ("a", "b", "z"))
    iso = [raw.get("iso", {}).get(i, form(c)) for i, c in enumerate(k.iso)]
    return keygen.KeygenParams(keygen._fe(a), keygen._fe(b), keygen._fe(z), ((ctypes.c_uint64 * 4) * 13)(*[keygen._fe(c) for c in iso]),
                               k.dst, len(k.dst), 1 if k.little_endian else 0)


def _call(lib, curve_id, label, label_len, n, kp, out, is_mont=False):
    return lib.reef_derive_generators(curve_id, label, label_len, n, None if kp is None else ctypes.byref(kp), is_mont,
                                      None if out is None else out.ctypes.data, 0)


def _still_works(curve):
    k = I.standin(curve)
    assert _ints(curve, _derive(curve, b"ck", 5, k)) == [_oracle_point(curve, b"ck", i) for i in range(5)]


@pytest.mark.parametrize("curve", CURVES)
def test_refused_arguments(curve, gpu_lib):
    cid = CURVES.index(curve)
    k = I.standin(curve)
    kp = _struct(k)
    out = np.zeros((8, 8), dtype=np.uint64)
    no_dst = _struct(k)
    no_dst.dst = None
    long_dst = _struct(I.with_params(k, dst=I.dst_of(256)))
    _still_works(curve)
    for what, args in (("n = 0", (b"ck", 2, 0, kp, out)), ("n = 2^27", (b"ck", 2, 1 << 27, kp, out)), ("null params", (b"ck", 2, 5, None, out)),
                       ("null out", (b"ck", 2, 5, kp, None)), ("null label", (None, 2, 5, kp, out)), ("null dst", (b"ck", 2, 5, no_dst, out)),
                       ("dst_len = 256", (b"ck", 2, 5, long_dst, out))):
        assert _call(gpu_lib, cid, *args) == REEF_ERR_ARG, what
        assert gpu_lib.reef_last_error() != b"" and not out.any(), what
        _still_works(curve)
    assert (no_dst.dst_len, long_dst.dst_len) == (len(k.dst), 256)
    assert _call(gpu_lib, cid, None, 0, 5, kp, out) == 0                               # a null label of no bytes is the empty label
    assert _ints(curve, out[:5]) == K.from_label(b"", 5, k)
    assert _call(gpu_lib, 7, b"ck", 2, 5, kp, out) != 0                                # no such curve
    _still_works(curve)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name,is_mont", (("a", False), ("a", True), ("z", False), ("z", True), ("iso[12]", False), ("iso[12]", True), ("b", True)))
def test_parameters_not_below_the_modulus_are_refused(curve, name, is_mont, gpu_lib):
    k = I.standin(curve)
    bad = {"a": dict(a=k.p), "z": dict(z=2 * k.p - 13), "iso[12]": dict(iso={12: R256 - 1}), "b": dict(b=k.p)}[name]
    out = np.zeros((5, 8), dtype=np.uint64)
    status = _call(gpu_lib, CURVES.index(curve), b"ck", 2, 5, _struct(k, is_mont, **bad), out, is_mont)
    message = gpu_lib.reef_last_error().decode()
    assert status == REEF_ERR_ARG and not out.any()
    assert f" {name} is not below the modulus" in message
    assert _call(gpu_lib, CURVES.index(curve), b"ck", 2, 5, _struct(k, is_mont), out, is_mont) == 0       # the same call with the element in range
    assert _ints(curve, out) == [_oracle_point(curve, b"ck", i) for i in range(5)]
