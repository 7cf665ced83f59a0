"""What several GPU test files share: uploads of the oracle's shapes and instances to a NIFS ctx, commitment keys, the named
Spartan and opening shapes, and the drivers that run a prove, a 3h opening or a 3i argument on the device call by call against
the reference's transcript.  The references themselves live under oracle/; nothing here is collected as a test."""
import random

import numpy as np

from oracle import pasta_ref
from oracle.ipa_oracle import compress, msm
from oracle.r1cs_oracle import field, layered_shape, to_mont
from oracle.spartan_oracle import Challenger, eq_evals, next_pow2
from reef_amd._fe import _arr


# ---------------------------------------------------------------------------------------------------------------- N6: NIFS
def upload_shape(nf, shape, is_mont):
    p = shape["p"]
    for k, m in enumerate("ABC"):
        r, c, v = shape[m]
        nf.set_matrix(k, r, c, _arr(to_mont(v, p) if is_mont else v), is_mont=is_mont)


def arr(vals, p, is_mont):
    return _arr(to_mont(vals, p) if is_mont else vals)


def set_running(nf, run, p, is_mont, zero_e=False):
    nf.set_running(arr(run["W"], p, is_mont), None if zero_e else arr(run["E"], p, is_mont), arr([run["u"]], p, is_mont),
                   arr(run["X"], p, is_mont), is_mont=is_mont)


def ap_key(curve, n):
    from reef_amd.msm import MsmContext
    bases = pasta_ref.gen_bases_ap(curve, 42, 5, n)
    return bases, MsmContext(curve, bases)


def key_of_kind(curve, gens, kind):
    from reef_amd.msm import MsmContext
    kw = {"pre": dict(bucket_groups=1, byte_tables=2), "tables": dict(bucket_groups=1, byte_tables=1), "plain": dict(bucket_groups=4)}[kind]
    key = MsmContext(curve, gens, **kw)
    assert key.has_byte_tables() == (kind == "tables")
    return key


# ---------------------------------------------------------------------------------------------------------------- N5: Spartan
def with_long_column(shape, col: int, seed: int) -> dict:
    """Adds to B, in every row, the pair (row, col, v), (row, col, -v): a column of 2 num_cons entries that sums to nothing."""
    p, rng = shape["p"], random.Random(seed)
    r, c, v = (list(x) for x in shape["B"])
    for i in range(shape["num_cons"]):
        x = rng.randrange(p)
        r += [i, i]
        c += [col, col]
        v += [x, (p - x) % p]
    return dict(shape, B=(r, c, v))


def pads_of(shape, pads):
    return pads or (next_pow2(shape["num_cons"]), next_pow2(max(shape["num_vars"], shape["num_io"] + 1)))


SPARTAN_SHAPES = {   # name: (layered_shape keyword arguments, (num_cons_pad, num_vars_pad) or None: the smallest legal)
    "smallest": (dict(num_cons=1, num_inputs=1, num_io=1), (2, 2)),
    "dup_empty": (dict(num_cons=127, dup_every=3, empty_every=5, extra_vars=4), None),
    "long_row": (dict(num_cons=300, long_row=1500, num_io=2), None),
    "vars_lt_cons": (dict(num_cons=500, num_inputs=3, empty_every=2, num_io=3), (512, 512)),      # u moves; num_vars_pad > num_vars
    "io_close": (dict(num_cons=100, num_inputs=4, num_io=120), None),                            # num_io = num_vars_pad - 8
    "cfg4": (dict(num_cons=39484, long_row=1100, empty_every=101, dup_every=13), (1 << 16, None)),
}


def spartan_shape(curve, name):
    kw, pads = SPARTAN_SHAPES[name]
    shape = layered_shape(curve, seed=len(name) + curve, **kw)
    if name == "cfg4":
        shape = with_long_column(shape, shape["num_vars"], 3)        # the u column: 2 x 39484 entries more
        pads = (pads[0], next_pow2(shape["num_vars"]))
    return shape, pads_of(shape, pads)


def prove_dev(nf, shape, pads, is_mont, seed):
    from reef_amd.spartan import prove
    return prove(nf, pads[0], pads[1], Challenger(shape["p"], seed), shape["p"], is_mont=is_mont)


PROOF_KEYS = ("tau", "outer", "r_x", "claims_outer", "r", "inner", "r_y", "claims_inner")


# ---------------------------------------------------------------------------------------------------------------- 3h: the opening
def opening_instances(curve, shape, inst, pf, gens):
    """[E, W] as 3h batches them, from the reference prove pf: {comm, a, b, eval}"""
    p = shape["p"]
    e1, e2 = eq_evals(pf["r_x"], p), eq_evals(pf["r_y"][1:], p)
    E, W = list(inst["E"]), list(inst["W"])
    out = []
    for a, b in ((E, e1), (W, e2)):
        out.append({"a": a, "b": b, "comm": msm(curve, gens[:len(a)], a) if a else np.zeros(12, np.uint64),
                    "eval": sum(x * y for x, y in zip(a, b)) % p})
    return out


def run_opening(nf, key, ref, curve, p, is_mont, trace=True):
    """The opening call by call with the reference's challenges: every output against the reference"""
    from reef_amd.spartan import Opening
    R = (1 << 256) % p
    to = (lambda v: v * R % p) if is_mont else (lambda v: v)
    frm = (lambda v: v * pow(R, -1, p) % p) if is_mont else (lambda v: v)
    op = Opening(nf)
    form = "Montgomery" if is_mont else "canonical"
    assert frm(op.begin(key, is_mont=is_mont)) == ref["cross"], f"cross term ({form})"
    assert frm(op.fold(to(ref["r"]), is_mont=is_mont)) == ref["c"], f"c ({form})"
    L, Rp = op.ipa_begin(ref["q"])
    assert (compress(curve, L), compress(curve, Rp)) == (compress(curve, ref["L"][0]), compress(curve, ref["R"][0])), f"L, R round 0 ({form})"
    for k, r in enumerate(ref["rs"][:-1]):
        L, Rp = op.ipa_round(to(r), is_mont=is_mont)
        assert compress(curve, L) == compress(curve, ref["L"][k + 1]), f"L round {k + 1} ({form})"
        assert compress(curve, Rp) == compress(curve, ref["R"][k + 1]), f"R round {k + 1} ({form})"
        if trace and (k < 3 or k == len(ref["rs"]) - 2):
            t = ref["trace"][k]
            assert [frm(v) for v in op.read(0, len(t["a"]), to_mont=is_mont)] == t["a"], f"a after round {k} ({form})"
            assert [frm(v) for v in op.read(1, len(t["b"]), to_mont=is_mont)] == t["b"], f"b after round {k} ({form})"
    assert frm(op.finish(to(ref["rs"][-1]), is_mont=is_mont)) == ref["a_hat"], f"a_hat ({form})"
    assert op.read(1, 1) == [ref["b_hat"]]
    return op


def open_shape(curve, name):
    """the Spartan shapes, and two with num_cons_pad and num_vars_pad apart (both padding directions)"""
    if name == "cons_gt_vars":
        shape = layered_shape(curve, 100, num_inputs=3, num_io=2, empty_every=9, seed=40 + curve)
        return shape, (512, pads_of(shape, None)[1])
    if name == "vars_gt_cons":
        shape = layered_shape(curve, 40, num_inputs=4, num_io=3, extra_vars=300, dup_every=4, seed=50 + curve)
        return shape, (64, 4 * pads_of(shape, None)[1])
    return spartan_shape(curve, name)


# ---------------------------------------------------------------------------------------------------------------- 3i: Hyrax
def hyrax_points(curve):
    return pasta_ref.gen_bases_ap(curve, 100003, 1, 1)[0], pasta_ref.gen_bases_ap(curve, 5003, 1, 1)[0]


def run_hyrax(hx, key, ref, curve, point, q, *, is_mont, h=None, blinds=None, trace=True):
    """The argument call by call with the reference's challenges: every output against the reference"""
    p = field(curve)
    R = (1 << 256) % p
    to = (lambda v: v * R % p) if is_mont else (lambda v: v)
    frm = (lambda v: v * pow(R, -1, p) % p) if is_mont else (lambda v: v)
    form = "Montgomery" if is_mont else "canonical"
    ev, lb = hx.eval_begin(key, [to(x) for x in point], is_mont=is_mont)
    assert (frm(ev), frm(lb)) == (ref["eval"], ref["lz_blind"]), f"eval, lz_blind ({form})"
    if trace:
        assert [frm(v) for v in hx.read(0, len(ref["lz"]), to_mont=is_mont)] == ref["lz"], f"a = LZ ({form})"
    bl = (lambda k: [to(x) for x in blinds[k]]) if h is not None else (lambda k: None)
    L, Rp = hx.ipa_begin(q, h, bl(0), is_mont=is_mont)
    assert (compress(curve, L), compress(curve, Rp)) == (compress(curve, ref["L"][0]), compress(curve, ref["R"][0])), f"L, R round 0 ({form})"
    for k, r in enumerate(ref["rs"][:-1]):
        L, Rp = hx.ipa_round(to(r), bl(k + 1), is_mont=is_mont)
        assert compress(curve, L) == compress(curve, ref["L"][k + 1]), f"L round {k + 1} ({form})"
        assert compress(curve, Rp) == compress(curve, ref["R"][k + 1]), f"R round {k + 1} ({form})"
        if trace and (k < 2 or k == len(ref["rs"]) - 2):
            t = ref["trace"][k]
            assert [frm(v) for v in hx.read(0, len(t["a"]), to_mont=is_mont)] == t["a"], f"a after round {k} ({form})"
            assert [frm(v) for v in hx.read(1, len(t["b"]), to_mont=is_mont)] == t["b"], f"b after round {k} ({form})"
    a_hat, b_hat = hx.finish(to(ref["rs"][-1]), is_mont=is_mont)
    assert (frm(a_hat), frm(b_hat)) == (ref["a_hat"], ref["b_hat"]), f"a_hat, b_hat ({form})"


def row_comms(curve, gens, z_ints, num_vars, left, row_blinds, h):
    rows, cols = 1 << left, 1 << (num_vars - left)
    zz = z_ints + [0] * ((1 << num_vars) - len(z_ints))
    out = []
    for i in range(rows):
        row = zz[i * cols:(i + 1) * cols]
        c = msm(curve, np.vstack([gens, h[None]]), row + [row_blinds[i]]) if row_blinds else msm(curve, gens, row)
        out.append(pasta_ref.to_affine(curve, c)[0])
    return np.stack(out)
