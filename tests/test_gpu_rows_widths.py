"""reef_msm_rows (K2) at every scalar width and on every route the width selects (v_msm_rows, reef_amd/csrc/engine.inc), on the adversarial
rows of tests/row_patterns.py: all ones (a carry through every window), the width on one lane of the last wave, every digit the top bucket
2^(c-1) (not negated) and 2^(c-1) + 1 (negated) for every window size 2..17, and uniform scalars.  Every result is compared bit-exactly, on
the compressed encoding, with the C oracle's cref.row_msm (itself checked on these rows by tests/test_rows_patterns.py).

The width is measured (max_scalar_bits = 0: k_max_bits), declared exactly (= b) and declared loosely (= 255); the tests never declare less than
the real width (the bound is trusted: undefined results, see MsmContext.msm_rows).  Scalars are canonical integers (is_mont = False) and, where said, v * 2^256 mod r
(is_mont = True: k_max_bits and k_recode convert first).

ROUTES, from the constants of engine.inc (MAX_LDS_KEYS = 32768, MAX_SCAN_KEYS = 4194304), bits = the width the engine works with:
  symbols     bits <= 8 and (tables cached for (bits, row_len) or rows * row_len >= 2 * table points): block tables, k_sym_entries
  single      bits + 1 <= 13: one signed window c = max(2, bits + 1), W = G = 1, table 0 only
  plain       bits + 1 > 13, key with one table (bucket_groups = 0): c = min(own choice, 11), W = G = ceil((bits + 1) / c)
  shifted     bits + 1 > 13, pre-shifted key: c, G the key's, W = min(key W, ceil((bits + 1) / c))
then, with keys_per_row = G * 2^(c-1) of that plan:
  sliced      rows > 1, row_len >= 8192, bits + 1 > 13: batches of rows through the K1 sort (k_count; the KEY's c and G, W cut as above)
  one-by-one  rows == 1, or keys_per_row > MAX_LDS_KEYS, or rows * keys_per_row > MAX_SCAN_KEYS: a K1 MSM per row at the key's full plan
              (k_recode_count with one bucket group, k_recode + k_count otherwise); the width is ignored
  LDS rows    everything else: k_recode, k_row_count, k_row_scatter; rows per workgroup = min(MAX_LDS_KEYS / keys_per_row, 65536 / row_len), 1 at least
"""
import numpy as np
import pytest

from oracle.pasta_oracle import CURVES
from row_patterns import batch, boundary_widths, to_limbs

pytestmark = pytest.mark.gpu
CID = {"pallas": 0, "vesta": 1}
SWEEP_ROWS, SWEEP_LEN = 5, 300


def mismatch(got: bytes, want: bytes):
    """None when equal; otherwise the rows that differ (row i of a batch is pattern ROW_PRIORITY[i % 5])."""
    if got == want:
        return None
    return [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]] or "length"


@pytest.fixture(scope="module")
def keys(cref):
    """Per curve: the longest key any test here needs (shorter ones are prefixes) and the blinding generator."""
    out = {}
    for name, cid in CID.items():
        out[name] = (cref.gen_bases_ap(cid, 77, 13, 70001), cref.gen_bases_ap(cid, 0xB11D, 1, 1)[0].copy())
    return out


@pytest.fixture(scope="module")
def ref(cref, keys):
    """case(name, b, rows, row_len, mont) -> (scalars, blinds, expected compressed rows with blinds): computed once per case and shared,
    never written to.  The oracle is given the same form of the scalars and blinds as the kernel (its `mont` flag)."""
    cache = {}

    def case(name, b, rows, row_len, mont=False):
        k = (name, b, rows, row_len, mont)
        if k not in cache:
            cid, r = CID[name], CURVES[name].order
            bases, h = keys[name]
            sc = to_limbs(batch(b, rows, row_len, r), r, mont)
            bl = cref.gen_scalars(cid, 0xB1 + b, rows, mont=mont)        # full-width blinds, in the scalars' form
            want = cref.compress(cid, cref.row_msm(cid, bases[:row_len].copy(), sc, rows, row_len, h=h, blinds=bl, mont=mont, threads=8))
            for a in (sc, bl):
                a.setflags(write=False)
            cache[k] = (sc, bl, want)
        return cache[k]
    return case


def run_widths(ctx, name, widths, rows, row_len, ref, keys, hints=(0, None, 255), mont_too=False):
    """Every width, every hint (None: the width itself): rows with blinds against the oracle."""
    from reef_amd import msm
    cid, h = CID[name], keys[name][1]
    for b in widths:
        sc, bl, want = ref(name, b, rows, row_len)
        for hint in hints:
            bits = b if hint is None else hint
            got = msm.compress(cid, ctx.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=bits, blinds=bl, h=h))
            assert mismatch(got, want) is None, (name, b, bits, "rows that differ", mismatch(got, want))
        if mont_too:
            msc, mbl, mwant = ref(name, b, rows, row_len, True)
            assert mwant == want                                           # the oracle agrees with itself across the two forms
            for bits in (0, b):
                got = msm.compress(cid, ctx.msm_rows(msc, rows, row_len, is_mont=True, max_scalar_bits=bits, blinds=mbl, h=h))
                assert mismatch(got, mwant) is None, (name, b, bits, "mont, rows that differ", mismatch(got, mwant))


# ------------------------------------------------------------------ the dense sweep: every b in 1..255 ----
# rows = 5 (the five patterns), row_len = 300: rows * row_len = 1500 never pays for symbol tables (b = 1: 2 * 34 * 2^9 table points) and
# no sweep context ever caches any, so b <= 12 is `single` (c = b + 1; b = 1: c = 2) and b >= 13 the key plan's route below; keys_per_row
# <= 4096 and 5 rows: always `LDS rows`, one workgroup (65536 / 300 = 218 rows per block at least 5).  max_scalar_bits = 255 runs the
# key's full plan at every b.
PLANS = {
    "a": dict(bucket_groups=0),                  # plain: b >= 13 -> c = min(choice for 300 points, 11), W = G = ceil((b + 1) / c)
    "b": dict(bucket_groups=1),                  # shifted, c = 13 (default for 300 points), G = 1: W = ceil((b + 1) / 13) of 20, cut at b = 13 k - 1 | 13 k
    "c": dict(window_bits=7, bucket_groups=1),   # shifted, c = 7, G = 1: W of 37, a cut every 7 bits
    "d": dict(window_bits=9, bucket_groups=4),   # shifted, c = 9, G = 4, 8 tables: W = ceil((b + 1) / 9) of 29; W < G for b = 13..26
}
CHUNKS = [(1, 52), (52, 103), (103, 154), (154, 205), (205, 256)]     # 51 widths a test: a few seconds each


@pytest.mark.parametrize("lo,hi", CHUNKS)
@pytest.mark.parametrize("name,plan", [("pallas", "a"), ("vesta", "a"), ("pallas", "b"), ("vesta", "b"), ("pallas", "c"), ("vesta", "d")])
def test_every_width_on_every_key_plan(name, plan, lo, hi, gpu_lib, cref, keys, ref):
    from reef_amd import msm
    with msm.MsmContext(CID[name], keys[name][0][:SWEEP_LEN].copy(), **PLANS[plan]) as ctx:
        p = ctx.plan()
        if plan == "a":
            assert p["tables"] == 1 and p["bucket_groups"] == p["windows"]
        else:
            assert (p["window_bits"], p["bucket_groups"]) == {"b": (13, 1), "c": (7, 1), "d": (9, 4)}[plan]
        run_widths(ctx, name, range(lo, hi), SWEEP_ROWS, SWEEP_LEN, ref, keys, mont_too=(plan == "b"))


# ------------------------------------------------------------------ routes the sweep does not reach ----
@pytest.mark.parametrize("name,rows,row_len,groups", [("pallas", 3, 8209, 1), ("vesta", 2, 70001, 0)])
def test_long_rows_of_narrow_scalars_through_the_lds_row_sort(name, rows, row_len, groups, gpu_lib, cref, keys, ref):
    """b in {9, 11, 12} (> 8: no symbol tables; b + 1 <= 13: `single`, c = b + 1, keys_per_row = 2^b <= 4096, not `sliced`) -> `LDS rows`.
    (3, 8209): min(32768 / 2^b, 65536 / 8209 = 7) >= 3 rows, one workgroup.  (2, 70001): 65536 / 70001 = 0 -> rows_per_block = 1, 70001 > 64Ki
    digits in one workgroup.  The hint 255 is the same batch as full-width rows: `sliced`, both rows one batch."""
    from reef_amd import msm
    with msm.MsmContext(CID[name], keys[name][0][:row_len].copy(), bucket_groups=groups) as ctx:
        run_widths(ctx, name, (9, 11, 12), rows, row_len, ref, keys)


@pytest.mark.parametrize("name,groups", [("pallas", 1), ("vesta", 0)])
def test_long_rows_through_the_sliced_batch_sort_at_window_boundaries(name, groups, gpu_lib, cref, keys, ref):
    """rows = 3, row_len = 8209 >= 8192, b >= 13 -> `sliced`: one batch of 3 (3 <= MAX_SCAN_KEYS / keys of the key, <= 64), run on the KEY's c
    and G with W = min(key W, ceil((b + 1) / c)); 3 MSMs in the batch -> k_recode + k_count + k_scatter.  groups = 1: shifted, G = 1;
    groups = 0: plain, G = the key's W > the W that is recoded.  Widths: the fixed boundaries and k c - 1, k c, k c + 1 for the key's own c."""
    from reef_amd import msm
    with msm.MsmContext(CID[name], keys[name][0][:8209].copy(), bucket_groups=groups) as ctx:
        c = ctx.plan()["window_bits"]
        run_widths(ctx, name, [b for b in boundary_widths(c) if b >= 13], 3, 8209, ref, keys)


def test_rows_too_wide_for_lds_go_one_by_one(gpu_lib, cref, keys, ref):
    """window_bits = 15, bucket_groups = 4: keys_per_row = 4 * 2^14 = 65536 > MAX_LDS_KEYS -> `one-by-one` for b >= 13 (rows = 3, row_len = 500 <
    8192), each row a K1 MSM at the key's full plan whatever the width (4 bucket groups: k_recode + k_count): the control.  b = 9, 12 are
    `single` (keys_per_row = 2^b) -> `LDS rows` on the same key."""
    from reef_amd import msm
    name = "pallas"
    with msm.MsmContext(CID[name], keys[name][0][:500].copy(), window_bits=15, bucket_groups=4) as ctx:
        assert (ctx.plan()["window_bits"], ctx.plan()["bucket_groups"]) == (15, 4)
        run_widths(ctx, name, boundary_widths(15), 3, 500, ref, keys)


@pytest.mark.parametrize("b", boundary_widths(13))
def test_more_rows_than_the_scan_holds_go_one_by_one(b, gpu_lib, cref, keys, ref):
    """bucket_groups = 1, c = 13 (default for 64 points): keys_per_row = 4096, rows = 1100 -> 1100 * 4096 = 4505600 > MAX_SCAN_KEYS -> `one-by-one` for
    b >= 12 (b = 12 is `single` with c = 13: the same 4096 keys a row), each row a K1 MSM with one bucket group (k_recode_count), the width
    ignored: the control.  b = 9: `single`, c = 10, 1100 * 512 keys -> `LDS rows`, 64 rows a workgroup, 18 workgroups, the last one ragged."""
    from reef_amd import msm
    name = "vesta"
    with msm.MsmContext(CID[name], keys[name][0][:64].copy(), bucket_groups=1) as ctx:
        assert (ctx.plan()["window_bits"], ctx.plan()["bucket_groups"]) == (13, 1)
        run_widths(ctx, name, [b], 1100, 64, ref, keys)


@pytest.mark.parametrize("where", ["last", "second-pass", "nowhere"])
def test_width_measured_past_the_grid_of_k_max_bits(where, gpu_lib, cref, keys):
    """rows = 1100, row_len = 480: N = 528000 > 2048 * 256 = 524288 threads, so k_max_bits strides.  One 40-bit scalar among zeros, at N - 1
    (thread 3711's second step, the last wave) or at 524288 + 5 (thread 5's second step): measured, bits = 40 -> shifted (window_bits = 7,
    G = 1, W = ceil(41 / 7) = 6), 1100 * 64 keys -> `LDS rows`.  A stride that lost it would measure 0 and recode one 2-bit window.
    All zero: measured 0 -> bits = 1, and 528000 >= 2 * 54 * 2^9 table points -> `symbols`: identity rows, or blind * H."""
    from reef_amd import msm
    name, rows, row_len = "pallas", 1100, 480
    cid, (bases, h) = CID[name], keys[name]
    N = rows * row_len
    sc = np.zeros((N, 4), dtype=np.uint64)
    if where != "nowhere":
        sc[N - 1 if where == "last" else 524288 + 5, 0] = (1 << 39) | 0x5A5A5A5A5
    bl = cref.gen_scalars(cid, 0xB1, rows, mont=False)
    kb = bases[:row_len].copy()
    want = cref.compress(cid, cref.row_msm(cid, kb, sc, rows, row_len, h=h, blinds=bl, mont=False, threads=8))
    want_nb = cref.compress(cid, cref.row_msm(cid, kb, sc, rows, row_len, mont=False, threads=8))
    if where == "nowhere":
        assert want_nb == bytes(32 * rows)
    else:
        assert want_nb.count(bytes(32)) >= rows - 1 and want_nb != bytes(32 * rows)      # only the 32 bytes of one row are not the identity's
    with msm.MsmContext(cid, kb, window_bits=7, bucket_groups=1) as ctx:
        for bits in (0, 40):
            assert mismatch(msm.compress(cid, ctx.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=bits)), want_nb) is None, bits
            assert mismatch(msm.compress(cid, ctx.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=bits, blinds=bl, h=h)), want) is None, bits


@pytest.mark.parametrize("name,rows,row_len", [("pallas", 37, 1000), ("vesta", 700, 300)])
def test_rows_of_zero_one_scalars(name, rows, row_len, gpu_lib, cref, keys, ref):
    """b = 1.  (37, 1000): 37000 < 2 * 112 * 2^9 table points -> `single` with c = max(2, 2) = 2, one bucket a row -> `LDS rows`, 37 rows in one
    workgroup (65536 / 1000 = 65).  (700, 300): 210000 >= 2 * 34 * 2^9 -> `symbols` (blocks of 9 bits); the hint 255 keeps both off the tables."""
    from reef_amd import msm
    with msm.MsmContext(CID[name], keys[name][0][:row_len].copy(), bucket_groups=1) as ctx:
        run_widths(ctx, name, [1], rows, row_len, ref, keys, mont_too=True)


def test_symbol_table_cache_sequence_on_one_context(gpu_lib, cref, keys, ref):
    """The tables a context caches are keyed by (bits, row_len); which route a narrow batch takes depends on them.  One context, in order, every
    call measured (hint 0) and then declared (hint b):"""
    from reef_amd import msm
    name = "pallas"
    cid, (bases, h) = CID[name], keys[name]

    def call(ctx, sc, bl, rows, row_len, b, want, step):
        for bits in (0, b):
            got = msm.compress(cid, ctx.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=bits, blinds=bl, h=h))
            assert mismatch(got, want) is None, (step, bits, mismatch(got, want))

    big3 = ref(name, 3, 600, 500)
    small3 = ref(name, 3, 4, 500)
    small4 = ref(name, 4, 4, 500)
    small12 = ref(name, 12, 4, 500)
    # the first batch's symbols at a 300-column prefix of every row
    pre_sc = np.ascontiguousarray(big3[0].reshape(600, 500, 4)[:, :300].reshape(-1, 4))
    assert max(int(x) for x in pre_sc[:, 0]) == 7 and not pre_sc[:, 1:].any()
    pre_want = cref.compress(cid, cref.row_msm(cid, bases[:300].copy(), pre_sc, 600, 300, h=h, blinds=big3[1], mont=False, threads=8))
    with msm.MsmContext(cid, bases[:500].copy(), bucket_groups=1) as ctx:
        call(ctx, big3[0], big3[1], 600, 500, 3, big3[2], 1)        # 300000 >= 2 * 167 * 2^9: `symbols`, builds the tables for (3, 500)
        call(ctx, small3[0], small3[1], 4, 500, 3, small3[2], 2)    # 2000 would not pay, but (3, 500) is cached: `symbols`
        call(ctx, small4[0], small4[1], 4, 500, 4, small4[2], 3)    # 4 bits: not cached, 2000 < 2 * 250 * 2^8: `single` c = 5, `LDS rows`; the cache stays
        call(ctx, small3[0], small3[1], 4, 500, 3, small3[2], 4)    # still cached: `symbols`
        call(ctx, pre_sc, big3[1], 600, 300, 3, pre_want, 5)        # (3, 300) is another key, 180000 >= 2 * 100 * 2^9: `symbols`, REBUILDS the tables
        call(ctx, small12[0], small12[1], 4, 500, 12, small12[2], 6)   # 12 bits: `single` c = 13, `LDS rows`
        call(ctx, big3[0], big3[1], 600, 500, 3, big3[2], 7)        # (3, 500) again: rebuilt once more
        call(ctx, small3[0], small3[1], 4, 500, 3, small3[2], 8)    # and cached again for the batch that does not pay


def test_group_rows_at_the_single_window_boundary(gpu_lib, cref, keys, ref):
    """Three members on device 0, split by window: 7 rows are dealt out whole in blocks of 2, 2 and 3, each member running reef_msm_rows on its block
    with the caller's hint, or measuring its OWN block's width (hint 0: only the first block holds the "ones" row).  Default group key: shifted,
    c = 13, G = 1.  b = 12: `single` c = 13; b = 13: W = 2; b = 26, 27: W = 3 (27 = the first width with a carry into a third window)."""
    from reef_amd import msm
    name, rows, row_len = "pallas", 7, 300
    cid, (bases, h) = CID[name], keys[name]
    with msm.MsmGroup(cid, bases[:row_len].copy(), [0, 0, 0], split=msm.SPLIT_WINDOWS) as g:
        for b in (12, 13, 26, 27):
            sc, bl, want = ref(name, b, rows, row_len)
            for bits in (0, b, 255):
                got = msm.compress(cid, g.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=bits, blinds=bl, h=h))
                assert mismatch(got, want) is None, (b, bits, mismatch(got, want))
