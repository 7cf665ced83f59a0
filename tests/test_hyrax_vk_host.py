"""The verifier's key of a committed document (include/reef_msm.h 3n) without a GPU: the three symbols in both libraries, the header,
the binding and INTEGRATION.md's Rust block; the argument checks that need no device; and the grouping of `verify_eval_batch` --
one `HyraxVk.comm_lz` call per vk, its encodings in the transcript, everything else as the row_comms32 route -- with the device
calls stubbed."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from abi_text import ROOT, header_prototypes, rust_kind, split_top, strip_comments
from reef_amd import _ffi, verify

NAMES = ("reef_hyrax_vk_create", "reef_hyrax_vk_destroy", "reef_hyrax_vk_comm_lz")
P = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001        # Pallas' scalar field


def test_symbols_are_exported_declared_and_bound_as_the_header_says():
    for path in (_ffi.LIB_PATH, _ffi.EXPERIMENT_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(raw, name), (path, name)
    declared = _ffi.declared_symbols()
    protos = header_prototypes()
    lib = _ffi.load()
    kinds = {None: "void", ctypes.c_int: "i32", ctypes.c_bool: "bool", ctypes.c_size_t: "usize", ctypes.c_void_p: "ptr"}
    for name in NAMES:
        assert name in declared and name in protos, name
        fn = getattr(lib, name)
        got = (kinds[fn.restype], [kinds.get(t, "ptr" if hasattr(t, "contents") else t) for t in fn.argtypes])
        assert got == protos[name], f"{name}: _ffi.py declares {got}, the header {protos[name]}"
    assert protos["reef_hyrax_vk_create"] == ("i32", ["ptr", "i32", "ptr", "usize", "i32", "i32", "ptr"])
    assert protos["reef_hyrax_vk_comm_lz"] == ("i32", ["ptr", "ptr", "usize", "bool", "ptr", "ptr"])
    assert protos["reef_hyrax_vk_destroy"] == ("void", ["ptr"])
    assert lib.reef_abi_version() == 7, "symbols added, none changed: the ABI version stays"


def test_the_rust_block_parses_against_the_header():
    protos = header_prototypes()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    seen = set()                                                      # (array types such as [u8; 32] hold a semicolon: the pattern lets them through)
    for m in re.finditer(r"\bfn\s+(reef_hyrax_vk_\w+)\s*\(((?:\[[^\]]*\]|[^;{}])*?)\)\s*(?:->\s*([^;{]+?))?\s*;", doc, flags=re.S):
        name, args, ret = m.group(1), strip_comments(m.group(2)), (m.group(3) or "void").strip()
        got = (rust_kind(ret), [rust_kind(a.split(":", 1)[1]) for a in split_top(args)])
        assert got == protos[name], f"{name}: INTEGRATION.md declares {got}, the header {protos[name]}"
        seen.add(name)
    assert seen == set(NAMES)
    assert "ReefHyraxVk" in doc


def test_argument_errors_that_need_no_device():
    lib = _ffi.load()
    rows = np.zeros(64, np.uint8)
    assert lib.reef_hyrax_vk_create(None, 0, rows.ctypes.data, 1, 0, -1, None) == 1                    # no place for the handle
    h = ctypes.c_void_p()
    assert lib.reef_hyrax_vk_create(ctypes.byref(h), 5, rows.ctypes.data, 1, 0, -1, None) == 1 and not h.value
    assert b"curve" in lib.reef_last_error()
    sentinel = np.full(12, 7, np.uint64)
    pts = np.zeros((1, 4), np.uint64)
    assert lib.reef_hyrax_vk_comm_lz(None, pts.ctypes.data, 1, False, sentinel.ctypes.data, None) == 1   # no vk
    assert (sentinel == 7).all()
    lib.reef_hyrax_vk_destroy(None)
    for left in (0, 26, -1):
        with pytest.raises(_ffi.ReefError, match="1 .. 25") as e:
            verify.HyraxVk(0, bytes(64), left)
        assert e.value.status == 1
    with pytest.raises(ValueError, match="4 row commitments of 32 bytes, got 96 bytes"):
        verify.HyraxVk(0, bytes(96), 2)
    with pytest.raises(ValueError):
        verify.HyraxVk("bn254", bytes(64), 1)
    vk = _stub_vk(0, 3, [])
    with pytest.raises(ValueError, match="point 1 has 2 entries"):
        verify.HyraxVk.comm_lz(vk, [[1, 2, 3], [1, 2]])
    jac, enc = verify.HyraxVk.comm_lz(vk, [])                         # no points: no call is made (the stub has no handle)
    assert jac.shape == (0, 12) and enc == []


# ---------------------------------------------------------------------------------------------------- verify_eval_batch's grouping
def _stub_vk(curve, left, log, tag=1):
    """a HyraxVk without a library handle whose comm_lz records its calls and answers with points that name (vk, point)"""
    vk = verify.HyraxVk.__new__(verify.HyraxVk)
    vk.curve, vk.left, vk._h, vk._lib = curve, left, None, None

    def comm_lz(points, compressed=True, *, is_mont=False):
        log.append((id(vk), [list(pt) for pt in points]))
        jac = np.array([[tag, sum(pt) % (1 << 63)] + [0] * 10 for pt in points], dtype=np.uint64).reshape(-1, 12)
        return jac, [b"vk%d:" % tag + int(sum(pt) % (1 << 63)).to_bytes(8, "little") for pt in points]
    vk.comm_lz = comm_lz
    return vk


def _instance(i, left, right, **route):
    point = [100 * i + j for j in range(left + right)]
    z = np.zeros(12, np.uint64)
    proof = {"L": [z] * right, "R": [z] * right, "a_hat": 5 + i, "rs": [2 + i] * right}
    return dict(q=np.zeros(8, np.uint64), point=point, left=left, eval=11 * i, proof=proof, **route)


def test_verify_eval_batch_groups_its_instances_by_vk(monkeypatch):
    left, right = 3, 2
    key = types.SimpleNamespace(curve=0)
    rows_calls, compress_calls, log_a, log_b = [], [], [], []

    def fake_comm_lz(curve, row_comms32, point_left, p):
        rows_calls.append((bytes(row_comms32), list(point_left)))
        return np.array([9, sum(point_left)] + [0] * 10, dtype=np.uint64)

    def fake_compress(k, pt):
        compress_calls.append(np.asarray(pt).copy())
        return b"c:" + np.asarray(pt, dtype=np.uint64).tobytes()[:16]
    monkeypatch.setattr(verify, "comm_lz", fake_comm_lz)
    monkeypatch.setattr(verify, "compress", fake_compress)
    vk_a, vk_b = _stub_vk(0, left, log_a, 1), _stub_vk(0, left, log_b, 2)
    insts = [_instance(0, left, right, vk=vk_a), _instance(1, left, right, row_comms32=b"r" * 256), _instance(2, left, right, vk=vk_b),
             _instance(3, left, right, vk=vk_a), _instance(4, left, right, vk=vk_a)]
    seen = {}

    def weights(absorbed):
        seen["absorbed"] = absorbed
        return [3 + i for i in range(len(absorbed))]

    def check_fn(k, n, proofs, rho, each=False):
        seen.update(n=n, proofs=proofs, rho=rho)
        return {"accept": True, "each": [True] * len(proofs)}
    assert verify.verify_eval_batch(key, insts, P, weights, each=True, check_fn=check_fn) == (True, [True] * 5)
    # ONE call per vk, with the points of its instances in their order; the rows route is called for its instance alone
    assert log_a == [(id(vk_a), [insts[i]["point"][:left] for i in (0, 3, 4)])]
    assert log_b == [(id(vk_b), [insts[2]["point"][:left]])]
    assert rows_calls == [(b"r" * 256, insts[1]["point"][:left])]
    # the transcript takes the vk's encodings as they came; comm_LZ is compressed for the rows instance only (and every L, R as before)
    firsts = [item[0] for item in seen["absorbed"]]
    assert firsts[0] == b"vk1:" + sum(insts[0]["point"][:left]).to_bytes(8, "little")
    assert firsts[2] == b"vk2:" + sum(insts[2]["point"][:left]).to_bytes(8, "little")
    assert firsts[3] == b"vk1:" + sum(insts[3]["point"][:left]).to_bytes(8, "little") and firsts[1].startswith(b"c:")
    assert sum(1 for c in compress_calls if c.reshape(-1)[0] == 9) == 1 and len(compress_calls) == 1 + 5 * 2 * right
    # each proof carries the comm_LZ of its own instance, then everything as the rows route passes it on
    assert [int(pr["comm"][1]) for pr in seen["proofs"]] == [sum(it["point"][:left]) for it in insts]
    assert [pr["c"] for pr in seen["proofs"]] == [it["eval"] % P for it in insts] and seen["n"] == 1 << right and seen["rho"] == [3, 4, 5, 6, 7]
    assert [pr["points"] for pr in seen["proofs"]] == [[it["point"][left:]] for it in insts]


def test_verify_eval_batch_refuses_a_vk_that_does_not_fit(monkeypatch):
    left, right = 3, 2
    key = types.SimpleNamespace(curve=0)
    weights = lambda absorbed: [1] * len(absorbed)                    # noqa: E731
    with pytest.raises(ValueError, match="instance 0: the vk is over 2\\^4 rows"):
        verify.verify_eval_batch(key, [_instance(0, left, right, vk=_stub_vk(0, 4, []))], P, weights)
    with pytest.raises(_ffi.ReefError, match="instance 0: the vk is of curve 1"):
        verify.verify_eval_batch(key, [_instance(0, left, right, vk=_stub_vk(1, left, []))], P, weights)
    with pytest.raises(ValueError, match="in place of"):
        verify.verify_eval_batch(key, [_instance(0, left, right, vk=_stub_vk(0, left, []), row_comms32=b"r" * 256)], P, weights)
    assert verify.verify_eval_batch(key, [], P, weights) is True


def test_verify_eval_takes_a_vk_in_place_of_the_rows(monkeypatch):
    left, right = 3, 2
    key = types.SimpleNamespace(curve=0)
    log = []
    vk = _stub_vk(0, left, log)
    monkeypatch.setattr(verify, "comm_lz", lambda *a: pytest.fail("the rows route was taken"))
    it = _instance(1, left, right)
    got = {}

    def check_fn(k, n, comm, c, q, L, R, rs, a_hat, points, wts, h=None, blind=None):
        got.update(comm=comm, c=c, points=points)
        return {"accept": True}
    assert verify.verify_eval(key, it["q"], vk, it["point"], left, it["eval"], it["proof"], P, check_fn=check_fn) is True
    assert log == [(id(vk), [it["point"][:left]])] and int(got["comm"][1]) == sum(it["point"][:left]) and got["points"] == [it["point"][left:]]
