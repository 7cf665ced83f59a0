"""reef_hyrax_commit and reef_hyrax_eval_comm_own on the GPU (reef_amd.hyrax over include/reef_msm.h 3i): the row commitments of a
resident document from its own ctx, byte for byte against gpu_drivers.row_comms encoded with the oracle's compress -- full, ragged,
short and empty documents, symbols of 1 / 2 / 4 bytes and field elements in both forms, both curves, with and without row blinds;
a row of zeros; documents that set the measured symbol width from one entry; more than one block of rows; the three key kinds; the
outputs in device memory or not taken at all; comm_LZ over the ctx's own rows; a whole argument on its own commitment through the
reference verifier; a commit between two IPA rounds; the errors, each with the ctx still usable."""
import random

import numpy as np
import pytest

from gpu_drivers import hyrax_points, key_of_kind, row_comms, run_hyrax
from oracle.hyrax_oracle import blind_total, hyrax_ref, jacobian, verify_hyrax
from oracle.ipa_oracle import compress, gens_of, msm
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import Challenger, eq_evals
from reef_amd._fe import _arr

pytestmark = pytest.mark.gpu

_SYM = {1: np.uint8, 2: np.uint16, 4: np.uint32}
NV, LEFT = 5, 2                                           # 4 rows x 8: the smallest shape where every branch exists


def _doc(curve, eb, n, seed, is_mont=False, below=None):
    """(what the device takes, the entries as ints): n symbols of eb bytes below `below` (default: the whole range), or field
    elements in the form is_mont names"""
    p = field(curve)
    r = random.Random(seed)
    if eb != 32:
        ints = [r.randrange(below or 1 << (8 * eb)) for _ in range(n)]
        return np.array(ints, dtype=np.uint64).astype(_SYM[eb]), ints
    ints = [r.randrange(p) for _ in range(n)]
    return _arr([v * (1 << 256) % p for v in ints] if is_mont else ints), ints


def _symbols(eb, ints):
    return np.array(ints, dtype=np.uint64).astype(_SYM[eb])


def _encode(curve, rows):
    """affine rows (k, 8) -> k x 32 bytes, the oracle's encoding; (0, 0) is the identity"""
    return b"".join(compress(curve, jacobian(curve, r)) for r in rows)


def _expected(curve, gens, ints, num_vars, left, row_blinds, h):
    rc = row_comms(curve, gens, list(ints), num_vars, left, row_blinds, h)
    return rc, _encode(curve, rc)


def _blinds(curve, left, seed):
    p = field(curve)
    r = random.Random(seed)
    return [r.randrange(p) for _ in range(1 << left)]


def _check_commit(hx, key, curve, gens, ints, num_vars, left, row_blinds, h, what=""):
    rc, enc = _expected(curve, gens, ints, num_vars, left, row_blinds, h)
    got, aff = hx.commit(key, h if row_blinds else None, affine=True)
    assert got == enc, f"comms32 {what}"
    assert np.array_equal(aff, rc), f"comms_affine {what}"
    return rc, enc


# 1. the smallest shape: full, ragged last row, ragged plus a padding row, exactly two rows, one ragged row, one symbol, nothing
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("eb", [1, 2, 4, 32])
@pytest.mark.parametrize("blinded", [False, True])
def test_rows_equal_the_oracle_at_every_document_length(gpu_lib, curve, eb, blinded):
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    rows, cols = 1 << LEFT, 1 << (NV - LEFT)
    gens, _ = gens_of(curve, cols)
    _, h = hyrax_points(curve)
    rb = _blinds(curve, LEFT, 11 + curve) if blinded else None
    R = (1 << 256) % p
    with key_of_kind(curve, gens, "pre") as key:
        for n in (32, 27, 17, 16, 5, 1, 0):
            for is_mont in ((False, True) if eb == 32 else (False,)):
                z, ints = _doc(curve, eb, n, 100 * n + eb + curve, is_mont)
                blinds_in = [v * R % p for v in rb] if (rb and is_mont) else rb
                with HyraxEval(curve, z, NV, LEFT, row_blinds=blinds_in, is_mont=is_mont) as hx:
                    rc, enc = _check_commit(hx, key, curve, gens, ints, NV, LEFT, rb, h, f"n = {n}, is_mont = {is_mont}")
                if not blinded:
                    used = -(-n // cols)
                    assert enc[32 * used:] == bytes(32 * (rows - used)), f"padding rows, n = {n}"
                    assert not rc[used:].any(), f"padding rows, n = {n}"


# 2. a row of zeros in the middle of a full document
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("eb", [1, 32])
def test_a_row_of_zeros_is_the_identity(gpu_lib, curve, eb):
    from reef_amd.hyrax import HyraxEval
    cols = 1 << (NV - LEFT)
    gens, _ = gens_of(curve, cols)
    _, ints = _doc(curve, eb, 1 << NV, 5 + eb)
    holed = ints[:cols] + [0] * cols + ints[2 * cols:]
    with key_of_kind(curve, gens, "pre") as key:
        encs = []
        for v in (ints, holed):
            z = _symbols(eb, v) if eb != 32 else _arr(v)
            with HyraxEval(curve, z, NV, LEFT) as hx:
                encs.append(_check_commit(hx, key, curve, gens, v, NV, LEFT, None, None)[1])
    full, hole = encs
    assert hole[32:64] == bytes(32) and hole[:32] == full[:32] and hole[64:] == full[64:] and full[32:64] != bytes(32)


# 3. the width measure: documents whose width one entry sets, at either end of the resident symbols
WIDTH_CASES = {
    "u8_below_8": (1, 8, None),
    "u8_255_at_26": (1, 8, (26, 255)),
    "u8_255_at_0": (1, 8, (0, 255)),
    "u16_below_8": (2, 8, None),
    "u16_0x1ff": (2, 8, (13, 0x1FF)),
    "u32_all_ones_at_26": (4, 8, (26, 0xFFFFFFFF)),
}


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("case", sorted(WIDTH_CASES))
def test_the_measured_width_covers_the_largest_symbol(gpu_lib, curve, case):
    from reef_amd.hyrax import HyraxEval
    eb, below, spike = WIDTH_CASES[case]
    gens, _ = gens_of(curve, 1 << (NV - LEFT))
    _, h = hyrax_points(curve)
    _, ints = _doc(curve, eb, 27, 40 + eb, below=below)
    if spike:
        ints[spike[0]] = spike[1]
    rb = _blinds(curve, LEFT, 3)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, _symbols(eb, ints), NV, LEFT, row_blinds=rb) as hx:
        _check_commit(hx, key, curve, gens, ints, NV, LEFT, rb, h, case)
        _check_commit(hx, key, curve, gens, ints, NV, LEFT, rb, h, case + ", again (the width is kept)")


# 4. more than one block and more than one wave of rows: 32 x 128, 23 full rows, one of 56, 8 padding rows
@pytest.fixture(scope="module")
def tall():
    out = {}
    for curve in (0, 1):
        gens, _ = gens_of(curve, 128)
        _, h = hyrax_points(curve)
        rb = _blinds(curve, 5, 50 + curve)
        for eb in (1, 2):
            _, ints = _doc(curve, eb, 3000, 60 + eb + curve)
            out[curve, eb] = (gens, h, rb, ints, _expected(curve, gens, ints, 12, 5, rb, h))
    return out


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("eb", [1, 2])
def test_many_rows_with_padding_rows_and_blinds(gpu_lib, tall, curve, eb):
    from reef_amd.hyrax import HyraxEval
    gens, h, rb, ints, (rc, enc) = tall[curve, eb]
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, _symbols(eb, ints), 12, 5, row_blinds=rb) as hx:
        got, aff = hx.commit(key, h, affine=True)
    assert got == enc and np.array_equal(aff, rc)


# 5. key kinds
@pytest.mark.parametrize("curve", [0, 1])
def test_key_kinds_give_the_same_rows(gpu_lib, curve):
    """4 x 2^11 (the byte-table range of a key): two full rows, a ragged one, a padding row; the pre-shifted bucket key, byte tables, a
    plain key"""
    from reef_amd.hyrax import HyraxEval
    num_vars, left = 13, 2
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    _, h = hyrax_points(curve)
    rb = _blinds(curve, left, 55)
    z, ints = _doc(curve, 1, 2 * 2048 + 100, 56 + curve)
    _, enc = _expected(curve, gens, ints, num_vars, left, rb, h)
    with HyraxEval(curve, z, num_vars, left, row_blinds=rb) as hx:
        for kind in ("pre", "tables", "plain"):
            with key_of_kind(curve, gens, kind) as key:
                assert hx.commit(key, h) == enc, kind


# 6. output placement
@pytest.mark.parametrize("curve", [0, 1])
def test_outputs_in_device_memory_or_not_taken(gpu_lib, curve):
    from reef_amd.hyrax import HyraxEval
    from reef_amd.msm import DeviceBuffer
    p = field(curve)
    rows = 1 << LEFT
    gens, _ = gens_of(curve, 1 << (NV - LEFT))
    z, ints = _doc(curve, 2, 27, 77)
    rc, enc = _expected(curve, gens, ints, NV, LEFT, None, None)
    rng = random.Random(6)
    point = [rng.randrange(p) for _ in range(NV)]
    want = compress(curve, msm(curve, rc, eq_evals(point[:LEFT], p)))
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, NV, LEFT) as hx:
        d32, daff = DeviceBuffer(32 * rows), DeviceBuffer(64 * rows)
        hx.commit_to_device(key, None, d32, daff)
        assert d32.to_host((32 * rows,), np.uint8).tobytes() == enc
        assert np.array_equal(daff.to_host((rows, 8)), rc)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, NV, LEFT) as hx:
        hx.commit_to_device(key)                              # both outputs NULL: the rows are only kept
        hx.eval_begin(key, point)
        assert compress(curve, hx.eval_comm_own()) == want


# 7. comm_LZ over the ctx's own rows
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("blinded", [False, True])
@pytest.mark.parametrize("n", [32, 13])
def test_eval_comm_own_is_eval_comm_over_the_oracle_rows(gpu_lib, curve, blinded, n):
    """n = 13: two padding rows, identities without blinds -- the comms key then holds (0, 0) bases"""
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    gens, _ = gens_of(curve, 1 << (NV - LEFT))
    _, h = hyrax_points(curve)
    rb = _blinds(curve, LEFT, 70) if blinded else None
    z, ints = _doc(curve, 1, n, 70 + n)
    rc, enc = _expected(curve, gens, ints, NV, LEFT, rb, h)
    rng = random.Random(7 + n)
    point = [rng.randrange(p) for _ in range(NV)]
    want = compress(curve, msm(curve, rc, eq_evals(point[:LEFT], p)))
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, NV, LEFT, row_blinds=rb) as hx:
        assert hx.commit(key, h if blinded else None) == enc
        hx.eval_begin(key, point)
        own = compress(curve, hx.eval_comm_own())
        assert own == want
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, NV, LEFT, row_blinds=rb) as hx:
        hx.eval_begin(key, point)
        assert compress(curve, hx.eval_comm(rc)) == own


# 8. the argument on its own commitment
@pytest.mark.parametrize("curve", [0, 1])
def test_argument_on_its_own_commitment_passes_the_verifier(gpu_lib, curve):
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    right = NV - LEFT
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    rng = random.Random(80 + curve)
    point = [rng.randrange(p) for _ in range(NV)]
    rb = _blinds(curve, LEFT, 81)
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)]
    z, ints = _doc(curve, 1, 29, 82)
    ref = hyrax_ref(curve, gens, ints, NV, LEFT, point, q, Challenger(p, 8), p, row_blinds=rb, h=h, blinds=blinds)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, NV, LEFT, row_blinds=rb) as hx:
        hx.commit(key, h)
        ev, lb = hx.eval_begin(key, point)
        assert (ev, lb) == (ref["eval"], ref["lz_blind"])
        comm_lz = hx.eval_comm_own()
        Ls, Rs = [], []
        L, Rp = hx.ipa_begin(q, h, blinds[0])
        Ls.append(L), Rs.append(Rp)
        for k, r in enumerate(ref["rs"][:-1]):
            L, Rp = hx.ipa_round(r, blinds[k + 1])
            Ls.append(L), Rs.append(Rp)
        a_hat, b_hat = hx.finish(ref["rs"][-1])
    pf = {"L": Ls, "R": Rs, "rs": ref["rs"], "a_hat": a_hat}
    total = blind_total(lb, blinds, ref["rs"], p)
    verify_hyrax(curve, gens, q, comm_lz, ev, eq_evals(point[LEFT:], p), pf, p, h=h, lz_blind_total=total)
    assert (a_hat, b_hat) == (ref["a_hat"], ref["b_hat"])


# 9. no interference: a commit between ipa_round k and k + 1
@pytest.mark.parametrize("curve", [0, 1])
def test_commit_between_two_rounds_changes_nothing_of_the_argument(gpu_lib, curve):
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    num_vars, left = 6, 3
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    rng = random.Random(90 + curve)
    point = [rng.randrange(p) for _ in range(num_vars)]
    rb = _blinds(curve, left, 91)
    z, ints = _doc(curve, 2, 61, 92)
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)]     # the argument's h term shares h's table on the key ctx with the commit
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, 9), p, row_blinds=rb, h=h, blinds=blinds)
    _, enc = _expected(curve, gens, ints, num_vars, left, rb, h)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left, row_blinds=rb) as hx:
        assert hx.eval_begin(key, point) == (ref["eval"], ref["lz_blind"])
        L, Rp = hx.ipa_begin(q, h, blinds[0])
        assert (compress(curve, L), compress(curve, Rp)) == (compress(curve, ref["L"][0]), compress(curve, ref["R"][0]))
        for k, r in enumerate(ref["rs"][:-1]):
            L, Rp = hx.ipa_round(r, blinds[k + 1])
            assert (compress(curve, L), compress(curve, Rp)) == (compress(curve, ref["L"][k + 1]), compress(curve, ref["R"][k + 1])), k
            t = ref["trace"][k]
            before = (hx.read(0, len(t["a"])), hx.read(1, len(t["b"])))
            assert before == (t["a"], t["b"])
            assert hx.commit(key, h) == enc, f"commit after round {k}"
            assert (hx.read(0, len(t["a"])), hx.read(1, len(t["b"]))) == before
        assert hx.finish(ref["rs"][-1]) == (ref["a_hat"], ref["b_hat"])


# 10. the errors, each with the ctx still usable afterwards
def test_errors_leave_the_ctx_usable(gpu_lib):
    from reef_amd._ffi import REEF_DEVICE, ReefError, check
    from reef_amd.hyrax import HyraxEval
    from reef_amd.msm import DeviceBuffer
    curve = 0
    p = field(curve)
    rows, cols = 1 << LEFT, 1 << (NV - LEFT)
    gens, _ = gens_of(curve, cols)
    _, h = hyrax_points(curve)
    rb = _blinds(curve, LEFT, 10)
    z, ints = _doc(curve, 1, 27, 10)
    rc, enc = _expected(curve, gens, ints, NV, LEFT, rb, h)
    rc_plain, enc_plain = _expected(curve, gens, ints, NV, LEFT, None, None)
    rng = random.Random(10)
    point = [rng.randrange(p) for _ in range(NV)]
    L = eq_evals(point[:LEFT], p)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, NV, LEFT, row_blinds=rb) as hx, HyraxEval(curve, z, NV, LEFT) as plain:
        with pytest.raises(ReefError, match="reef_hyrax_eval_begin"):
            hx.eval_comm_own()                                # an order error: the point is not set
        hx.eval_begin(key, point)
        with pytest.raises(ReefError, match="reef_hyrax_commit"):
            hx.eval_comm_own()                                # never committed
        assert hx.commit(key, h) == enc
        own = compress(curve, hx.eval_comm_own())
        assert own == compress(curve, msm(curve, rc, L))

        def still_the_same():
            assert compress(curve, hx.eval_comm_own()) == own
        with key_of_kind(1, gens_of(1, cols)[0], "pre") as other, pytest.raises(ReefError, match="curve 1"):
            hx.commit(other, h)
        still_the_same()
        with key_of_kind(curve, gens_of(curve, 2 * cols)[0], "pre") as longer, \
                pytest.raises(ReefError, match=f"{2 * cols} points.*exactly 2\\^\\(num_vars - left_vars\\) = {cols}"):
            hx.commit(longer, h)
        still_the_same()
        with key_of_kind(curve, gens, "plain") as split:
            split.set_window_split(0, 2)
            with pytest.raises(ReefError, match="window split"):
                hx.commit(split, h)
        still_the_same()
        with pytest.raises(ReefError, match="row blinds"):
            hx.commit(key)                                    # blinds without h
        still_the_same()
        with pytest.raises(ReefError, match="no row blinds"):
            plain.commit(key, h)                              # h without blinds
        assert plain.commit(key) == enc_plain
        d32 = DeviceBuffer(32 * rows + 16)
        ha = np.ascontiguousarray(h, dtype=np.uint64)
        with pytest.raises(ReefError, match="16-byte aligned"):
            check(hx._lib.reef_hyrax_commit(hx._h, key._h, ha.ctypes.data, d32.ptr + 8, None, REEF_DEVICE))
        still_the_same()
        # the caller's rows replace the ctx's own
        assert compress(curve, hx.eval_comm(rc_plain)) == compress(curve, msm(curve, rc_plain, L))
        with pytest.raises(ReefError, match="reef_hyrax_commit"):
            hx.eval_comm_own()
        assert hx.commit(key, h) == enc                       # ... and commit makes them again
        still_the_same()
        hx.eval_comm_compressed(enc_plain)
        with pytest.raises(ReefError, match="reef_hyrax_commit"):
            hx.eval_comm_own()
