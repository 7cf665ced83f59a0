"""The resident Poseidon Merkle tree on the GPU (include/reef_msm.h 3d: reef_merkle_create / _info / _open / _read_level / _check_paths)
against the oracle, bit for bit: the stand-in constants of oracle.merkle_oracle, canonical integers on Pallas's scalar field and the pasta
Montgomery form on Vesta's.  The oracle's trees are computed once per (field, size) and shared (tests/merkle_drivers.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

from merkle_drivers import FIELDS, Raw, expected_open, limbs, oracle_tree, params, path_alterations
from oracle import merkle_oracle as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 100, 1001, 4097])
def test_every_index_against_the_oracle(n, curve, gpu_lib):
    from reef_amd import merkle
    doc, root, tree = oracle_tree(curve, n)
    t = Raw(curve, doc)
    try:
        assert (t.n, t.levels, t.nodes, t.root) == (n, len(tree), merkle.nodes(n), root)
        idx = list(range(n))
        st, sym, oidx, opp, path = t.open(idx)
        assert st == 0, t.error()
        esym, eoidx, eopp, epath = expected_open(doc, tree, idx)
        assert sym == esym and oidx == eoidx
        assert opp == eopp
        assert path == epath
        wits = merkle.wits_from_arrays(idx, n, t.levels, np.asarray(oidx, dtype=np.uint64), np.array([limbs(x) for x in opp], dtype=np.uint64))
        for q in idx:
            assert [tuple(w) for w in wits[q]] == [tuple(w) for w in M.path_wits(doc, tree, q)], q
        for h, level in enumerate(tree):
            st, got = t.read_level(h, 0, len(level))
            assert st == 0 and got == level, h
            first = len(level) // 3
            count = min(max(1, len(level) // 2), len(level) - first)
            st, got = t.read_level(h, first, count)
            assert st == 0 and got == level[first:first + count], (h, first, count)
            assert t.read_level(h, len(level), 1)[0] == 1 and t.read_level(h, 0, len(level) + 1)[0] == 1      # past the level's end
            assert t.read_level(h, len(level), 0)[0] == 0
        assert t.read_level(len(tree), 0, 1)[0] == 1
    finally:
        t.close()


def test_the_resident_tree_is_the_one_shot_tree(gpu_lib):
    from reef_amd import merkle
    from reef_amd.sumcheck import array_to_ints
    p = params("pallas")
    n = 4097
    doc = np.asarray([(31 * i + 7) % 131 for i in range(n)], dtype=np.uint32)
    root, levels = merkle.commit_arrays("pallas", doc, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node)
    with merkle.ResidentMerkleCommitment.new("pallas", doc, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node) as rm:
        assert rm.commitment == root and rm.levels == len(levels) and rm.nodes == sum(lv.shape[0] for lv in levels)
        for h, lv in enumerate(levels):
            assert rm.level(h) == array_to_ints(lv), h


def test_open_order_and_shape(gpu_lib):
    n = 4097
    doc, root, tree = oracle_tree("pallas", n)
    t = Raw("pallas", doc)
    try:
        rng = np.random.default_rng(11)
        big = [int(x) for x in rng.integers(0, n, size=1000)]                 # unsorted, with duplicates
        assert len(set(big)) < len(big)
        for idx in ([], [n - 1], [5, 5, 4096, 0, 5], big):
            st, sym, oidx, opp, path = t.open(idx)
            assert st == 0, t.error()
            assert (sym, oidx, opp, path) == expected_open(doc, tree, idx), len(idx)
        st, _, _, opp, _ = t.open(big, want_sym=False, want_oidx=False, want_path=False, fill=0xA5)
        assert st == 0 and opp == expected_open(doc, tree, big)[2]
        sym_raw, oidx_raw, _, path_raw = t.raw_out
        assert (sym_raw == 0xA5).all() and (oidx_raw == 0xA5).all() and (path_raw == 0xA5).all()    # NULL outputs: nothing else was written either
        st = t.open([0, 1, 2, n, 4, n + 7], fill=0xA5)[0]
        assert st == 1 and "idx[3]" in t.error(), t.error()
        assert all((a == 0xA5).all() for a in t.raw_out)                      # nothing written
        st = t.open([1 << 40])[0]
        assert st == 1 and "idx[0]" in t.error()
    finally:
        t.close()


def alterations(L):
    """(name, depth) of the fields of one opening that the check must notice: the issue's list, the depths deduplicated for short trees"""
    out = path_alterations(L)                                               # the symbol, the sibling's index, the sibling at three depths
    return out[:2] + [("idx_bit0", None)] + out[2:]


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
@pytest.mark.parametrize("n", [2, 1001])
def test_recomputing_the_root_from_openings(n, curve, gpu_lib):
    doc, root, tree = oracle_tree(curve, n)
    L = len(tree)
    t = Raw(curve, doc)
    try:
        for k in (1, 12, 13, 60, 61, 700):
            idx = [(5 * j + 3) % n for j in range(k)]
            sym, oidx, opp, _ = expected_open(doc, tree, idx)
            if k == 13:                                                       # the oracle agrees that these openings are honest (~1 ms a hash)
                for j in (0, 12):
                    wits = [((idx[j] >> h) & 1 == 0, oidx[j] if h == 0 else None, opp[j * L + h]) for h in range(L)]
                    assert M.root_from_path(doc, idx[j], wits, params(curve)) == root
            st, accept = t.check_paths(idx, sym, oidx, opp)
            assert st == 0 and accept == [1] * k, (k, t.error())
            for victim in sorted({k // 24 * 12 + min(5, (k - 1) // 2), k - 1}):   # the middle of a wave (of twelve paths); the last path
                for name, depth in alterations(L):
                    i2, s2, o2, p2 = list(idx), list(sym), list(oidx), list(opp)
                    if name == "symbols":
                        s2[victim] += 1
                    elif name == "opposite_idx":
                        o2[victim] += 1
                    elif name == "idx_bit0":
                        if (i2[victim] ^ 1) >= n:
                            continue                                          # the altered index would be out of range: an argument error, below
                        i2[victim] ^= 1
                    else:
                        p2[victim * L + depth] = (p2[victim * L + depth] + 1) % FIELDS[curve][0]
                    st, accept = t.check_paths(i2, s2, o2, p2)
                    assert st == 0, t.error()
                    assert accept == [0 if j == victim else 1 for j in range(k)], (k, victim, name, depth)
        idx = [0, n - 1]
        sym, oidx, opp, _ = expected_open(doc, tree, idx)
        raw = t.fe_array(opp)
        raw[L + L // 2] = limbs(FIELDS[curve][0])                             # the modulus itself, in whichever form: not below the modulus
        st, _ = t.check_paths(idx, sym, oidx, None, raw_opp=raw)
        assert st == 1 and f"opposite[{L + L // 2}]" in t.error(), t.error()
        st, _ = t.check_paths([0, n], sym, oidx, opp)
        assert st == 1 and "idx[1]" in t.error(), t.error()
        assert t.check_paths([], [], [], [])[0] == 0
    finally:
        t.close()


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_the_thread_per_path_form_of_the_check(curve, gpu_lib):
    """More paths than the five-lane form takes (POS_SPREAD_MAX_NODES = 16384, merkle_kernels.inc): 16385 paths of depth 3.  On Vesta the claimed
    siblings cross in Montgomery form."""
    n, k = 8, 16385
    doc, root, tree = oracle_tree(curve, n)
    L = len(tree)
    assert L == 3
    t = Raw(curve, doc)
    try:
        idx = [(3 * j + 1) % n for j in range(k)]
        sym, oidx, opp, _ = expected_open(doc, tree, idx)
        st, accept = t.check_paths(idx, sym, oidx, opp)
        assert st == 0 and accept == [1] * k, t.error()
        for victim, slot in ((k // 2, 1), (k - 1, 2), (0, 0)):
            p2 = list(opp)
            p2[victim * L + slot] = (p2[victim * L + slot] + 1) % FIELDS[curve][0]
            st, accept = t.check_paths(idx, sym, oidx, p2)
            assert st == 0 and accept.count(0) == 1 and accept[victim] == 0, (victim, slot)
        s2 = list(sym)
        s2[k - 1] += 1
        st, accept = t.check_paths(idx, s2, oidx, opp)
        assert st == 0 and accept.count(0) == 1 and accept[k - 1] == 0
    finally:
        t.close()


def test_lifetime_of_contexts(gpu_lib):
    from reef_amd import merkle, msm
    p = params("pallas")
    doc_a, root_a, tree_a = oracle_tree("pallas", 100)
    doc_b, root_b, tree_b = oracle_tree("pallas", 7, 13, 5)
    new = lambda d: merkle.ResidentMerkleCommitment.new("pallas", d, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node)   # noqa: E731
    a, b = new(doc_a), new(doc_b)
    assert (a.commitment, b.commitment) == (root_a, root_b)
    assert [tuple(w) for w in a.path_wits(99)] == [tuple(w) for w in M.path_wits(doc_a, tree_a, 99)]
    a.close()
    a.close()                                                                 # twice is once
    lookups = [6, 0, 3]
    wits = b.make_wits(lookups)
    assert [[tuple(w) for w in ws] for ws in wits] == [[tuple(w) for w in M.path_wits(doc_b, tree_b, q)] for q in lookups]
    assert b.check(lookups, wits) == [True, True, True]
    assert b.check(lookups, wits, symbols=[doc_b[6], doc_b[0] + 1, doc_b[3]]) == [True, False, True]
    sym, oidx, opp, path = b.open_arrays(lookups, want_path=True)
    assert sym.tolist() == [doc_b[q] for q in lookups] and path is not None and b.open_arrays(lookups)[3] is None
    assert b.level(len(tree_b) - 1) == [root_b] and b.level(0, 1, 2) == tree_b[0][1:3]
    with pytest.raises(IndexError):
        b.path_wits(7)
    b.close()
    a = new(doc_a)                                                            # create, destroy, create again
    assert a.commitment == root_a and a.level(1) == tree_a[1]
    a.close()
    with pytest.raises(msm.ReefError) as e:
        merkle.ResidentMerkleCommitment.new("pallas", doc_b, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node, device=99)
    assert e.value.status == 1 and "device" in str(e.value)
    with pytest.raises(msm.ReefError):
        merkle.ResidentMerkleCommitment.new("pallas", doc_b, 3, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node)              # reef_merkle_commit's errors


def test_the_cpp_front_end(gpu_lib):
    """host/merkle_resident_selftest.cpp: MerkleCommitmentResident of reef_provider.hpp on 1001 seeded symbols; every value it prints is the oracle's."""
    from reef_amd import _ffi
    exe = os.path.join(os.path.dirname(_ffi.LIB_PATH), "merkle_resident_selftest")
    assert os.path.exists(exe), "build() did not produce merkle_resident_selftest"
    run = subprocess.run([exe, "1001"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    n = 1001
    doc, root, tree = oracle_tree("pallas", n)
    L = len(tree)
    fhex = lambda x: x.to_bytes(32, "little").hex()                           # noqa: E731
    lookups = [0, 1, n // 2, n - 2, n - 1]
    assert (got["n"], got["root"], got["levels"], got["lookups"]) == (n, fhex(root), L, lookups)
    want = [[[w[0], w[1], fhex(w[2])] for w in M.path_wits(doc, tree, q)] for q in lookups]
    assert got["wits"] == want
    assert got["path"] == [fhex(tree[h][q >> (h + 1)]) for q in lookups for h in range(L)]
    assert got["single"] == want[2][-1][2]
    assert got["symbols"] == [doc[q] for q in lookups]
    assert got["accept"] == [1, 1, 1, 1, 1] and got["accept_altered"] == [1, 1, 0, 1, 0]
    assert got["oob_throws"] is True
    assert subprocess.run([exe, "0"], capture_output=True, text=True, timeout=60).returncode == 2
