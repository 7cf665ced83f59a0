"""The Hyrax consistency argument on the host (include/reef_msm.h 3i): the big-integer reference of oracle/hyrax_oracle.py checked by its
verifier -- honest transcripts with and without the per-round h blinds pass, a changed L, R, a_hat or challenge fails -- and against
oracle/mle_oracle.py for LZ and eval; the library's new symbols agree with their ctypes signatures and INTEGRATION 2i's Rust block."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from abi_text import header_prototypes, rust_kind, split_top, strip_comments
from oracle import mle_oracle, pasta_ref
from oracle.hyrax_oracle import blind_total, bound_ref, hyrax_ref, verify_hyrax
from oracle.ipa_oracle import gens_of, msm
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import Challenger, eq_evals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("reef_hyrax_create", "reef_hyrax_destroy", "reef_hyrax_eval_begin", "reef_hyrax_eval_comm", "reef_hyrax_ipa_begin",
           "reef_hyrax_ipa_round", "reef_hyrax_finish", "reef_hyrax_read")


def instance(curve: int, num_vars: int, n: int, seed: int, *, symbols: bool = False, blinded: bool = False):
    """A document of n entries (symbols < 2^8 or field elements), its row commitments over gens_v (+ blind_i h), a point"""
    p = field(curve)
    rng = random.Random(seed)
    left = num_vars // 2
    rows, cols = 1 << left, 1 << (num_vars - left)
    z = [rng.randrange(256) if symbols else rng.randrange(p) for _ in range(n)]
    gens, _ = gens_of(curve, cols)
    h = pasta_ref.gen_bases_ap(curve, 5003, 1, 1)[0]
    q = pasta_ref.gen_bases_ap(curve, 100003, 1, 1)[0]
    row_blinds = [rng.randrange(p) for _ in range(rows)] if blinded else None
    zz = z + [0] * ((1 << num_vars) - n)
    comms = []
    for i in range(rows):
        row = zz[i * cols:(i + 1) * cols]
        if blinded:
            c = msm(curve, np.vstack([gens, h[None]]), row + [row_blinds[i]])
        else:
            c = msm(curve, gens, row)
        comms.append(pasta_ref.to_affine(curve, c)[0])
    point = [rng.randrange(p) for _ in range(num_vars)]
    return {"z": z, "left": left, "gens": gens, "h": h, "q": q, "row_blinds": row_blinds, "row_comms": np.stack(comms), "point": point}


def prove(curve: int, inst: dict, num_vars: int, seed: int, *, round_blinds: bool):
    p = field(curve)
    rng = random.Random(seed + 7)
    right = num_vars - inst["left"]
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)] if round_blinds else None
    pf = hyrax_ref(curve, inst["gens"], inst["z"], num_vars, inst["left"], inst["point"], inst["q"], Challenger(p, seed), p,
                   row_blinds=inst["row_blinds"], h=inst["h"] if round_blinds else None, blinds=blinds, row_comms=inst["row_comms"])
    return pf, blinds


def verify(curve: int, inst: dict, num_vars: int, pf: dict, blinds) -> None:
    p = field(curve)
    b0 = eq_evals(inst["point"][inst["left"]:], p)
    blinded = blinds is not None or inst["row_blinds"] is not None
    total = blind_total(pf["lz_blind"], blinds or [], pf["rs"], p)
    verify_hyrax(curve, inst["gens"], inst["q"], pf["comm_lz"], pf["eval"], b0, pf, p, h=inst["h"] if blinded else None,
                 lz_blind_total=total)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("num_vars", [2, 3, 5, 8])
@pytest.mark.parametrize("mode", ["plain", "row_blinds", "round_blinds"])
def test_reference_argument_satisfies_the_verifier(curve, num_vars, mode):
    n = (1 << num_vars) - (num_vars % 3)                          # a zero-padded tail on some shapes
    inst = instance(curve, num_vars, n, 10 * num_vars + curve, symbols=num_vars % 2 == 1, blinded=mode != "plain")
    pf, blinds = prove(curve, inst, num_vars, num_vars, round_blinds=mode == "round_blinds")
    assert len(pf["L"]) == num_vars - inst["left"] and len(pf["trace"][-1]["a"]) == 1
    p = field(curve)
    assert pf["eval"] == mle_oracle.evaluate(inst["z"], inst["point"], p)
    verify(curve, inst, num_vars, pf, blinds)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("what", ["L", "R", "a_hat", "challenge"])
@pytest.mark.parametrize("round_blinds", [False, True])
def test_tampering_fails_the_verifier(curve, what, round_blinds):
    p, num_vars = field(curve), 6
    inst = instance(curve, num_vars, 1 << num_vars, 3 + curve, blinded=round_blinds)
    pf, blinds = prove(curve, inst, num_vars, 5, round_blinds=round_blinds)
    verify(curve, inst, num_vars, pf, blinds)
    pf = dict(pf, L=list(pf["L"]), R=list(pf["R"]), rs=list(pf["rs"]))
    if what in ("L", "R"):
        pf[what][1] = msm(curve, np.stack([pasta_ref.to_affine(curve, pf[what][1])[0], inst["gens"][0]]), [1, 1])
    elif what == "a_hat":
        pf["a_hat"] = (pf["a_hat"] + 1) % p
    else:
        pf["rs"][1] = (pf["rs"][1] + 1) % p
    with pytest.raises(AssertionError, match="P_hat"):
        verify(curve, inst, num_vars, pf, blinds)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("num_vars,left", [(2, 1), (5, 2), (9, 4), (10, 5), (11, 3)])
def test_bound_rows_agree_with_the_mle_oracle(curve, num_vars, left):
    p = field(curve)
    rng = random.Random(num_vars * 31 + left)
    z = [rng.randrange(p) for _ in range((1 << num_vars) - 3)]
    point = [rng.randrange(p) for _ in range(num_vars)]
    assert bound_ref(z, num_vars, left, point, p) == mle_oracle.bound_rows(z, point, left, p)
    lz, ev = bound_ref(z, num_vars, left, point, p)
    assert ev == mle_oracle.evaluate(z, point, p)
    assert sum(a * b for a, b in zip(lz, eq_evals(point[left:], p))) % p == ev


def test_lz_blind_is_the_blinds_as_a_one_column_table():
    p = field(0)
    rng = random.Random(9)
    blinds = [rng.randrange(p) for _ in range(8)]
    point = [rng.randrange(p) for _ in range(5)]
    lz, ev = bound_ref(blinds, 3, 3, point[:3], p)
    assert lz == [sum(a * b for a, b in zip(eq_evals(point[:3], p), blinds)) % p] and ev == lz[0]


_CTYPES = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_size_t: "usize", ctypes.c_bool: "bool", None: "void"}


def _ctypes_kind(t):
    if t in _CTYPES:
        return _CTYPES[t]
    return "ptr" if issubclass(t, (ctypes._Pointer, ctypes.c_void_p)) else str(t)


def test_header_ctypes_and_integration_agree_on_the_new_symbols():
    from reef_amd import _ffi
    lib = _ffi.load()
    protos = header_prototypes()
    for name in SYMBOLS:
        assert name in protos and name in _ffi.declared_symbols(), name
        fn = getattr(lib, name)
        got = (_ctypes_kind(fn.restype), [_ctypes_kind(a) for a in fn.argtypes])
        assert got == protos[name], f"{name}: ctypes {got}, header {protos[name]}"
    assert lib.reef_abi_version() == _ffi.ABI_VERSION == 7
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 2i\b.*?(?=^## )", doc, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no section 2i"
    block = m.group(0)
    seen = set()
    for f in re.finditer(r"\bfn\s+(reef_hyrax_\w+)\s*\(((?:[^;{}()\[\]]|\[[^\]]*\])*?)\)\s*(?:->\s*([^;{]+?))?\s*;", block, flags=re.S):
        name, args, ret = f.group(1), strip_comments(f.group(2)), (f.group(3) or "void").strip()
        got = (rust_kind(ret), [rust_kind(a.split(":", 1)[1]) for a in split_top(args)])
        assert got == protos[name], f"{name}: INTEGRATION 2i {got}, header {protos[name]}"
        seen.add(name)
    assert seen == set(SYMBOLS), sorted(set(SYMBOLS) - seen)


def test_documents_of_the_wrong_kind_are_refused_on_the_host():
    from reef_amd.hyrax import _table
    assert _table(np.zeros(8, np.uint16))[2:] == (8, 2)
    assert _table(np.zeros(8, np.int32))[2:] == (8, 4)
    assert _table(np.zeros((8, 4), np.uint64))[2:] == (8, 32)
    for bad in (np.zeros(16, np.int64), np.zeros(16, np.int8), np.zeros(16, np.float32), np.zeros((8, 2), np.uint64),
                np.zeros((4, 8), np.uint64).T, np.zeros(32, np.uint8)[::2], [1, 2, 3]):
        with pytest.raises((TypeError, ValueError)):
            _table(bad)
