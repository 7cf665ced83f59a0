"""The host half of the resident Merkle tree (reef_amd/merkle.py: wits_from_arrays): reef_merkle_open's arrays, fabricated here from
the oracle's tree, turn into the MerkleWit lists of the oracle's path_wits, and those recompute the root.  No GPU."""
import numpy as np
import pytest

from oracle import merkle_oracle as M
from reef_amd import _ffi
from reef_amd.merkle import wits_from_arrays
from reef_amd.sumcheck import ints_to_array

P = M.standin_params()


def open_arrays_of(doc, tree, idx):
    """What reef_merkle_open writes for `idx` (include/reef_msm.h 3d), from the oracle's tree alone: opposite_idx (k), opposite (k * L)."""
    n, L = len(doc), len(tree)
    oidx, opp = [], []
    for q in idx:
        sib = q ^ 1
        have = sib < n
        oidx.append(sib if have else 0)
        opp.append(doc[sib] if have else 0)
        for h in range(L - 1):
            s = (q >> (h + 1)) ^ 1
            opp.append(tree[h][s] if s < len(tree[h]) else 0)
    return np.asarray(oidx, dtype=np.uint64), ints_to_array(opp)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 1001])
def test_wits_from_arrays_are_the_oracles_path_wits(n):
    doc = [(31 * i + 7) % 131 for i in range(n)]
    root, tree = M.commit(doc, P)
    idx = list(range(n))
    oidx, opp = open_arrays_of(doc, tree, idx)
    wits = wits_from_arrays(idx, n, len(tree), oidx, opp)
    assert len(wits) == n
    for q, w in zip(idx, wits):
        assert [tuple(x) for x in w] == [tuple(x) for x in M.path_wits(doc, tree, q)], q
    for q in sorted({0, n // 2, n - 1} if n > 8 else set(idx)):          # the oracle's sponge takes ~1 ms a hash
        assert M.root_from_path(doc, q, wits[q], P) == root, q


def test_wits_from_arrays_refuses_what_does_not_fit():
    doc = [2, 3, 4, 5, 6, 7, 8]
    _, tree = M.commit(doc, P)
    oidx, opp = open_arrays_of(doc, tree, [0, 6])
    with pytest.raises(IndexError):
        wits_from_arrays([0, 7], 7, len(tree), oidx, opp)
    with pytest.raises(ValueError):
        wits_from_arrays([0, 6], 7, len(tree) + 1, oidx, opp)
    assert wits_from_arrays([], 7, len(tree), oidx[:0], opp[:0]) == []


def test_the_header_declares_the_resident_entry_points_and_the_binding_binds_them():
    names = set(_ffi.declared_symbols())
    new = {"reef_merkle_create", "reef_merkle_destroy", "reef_merkle_info", "reef_merkle_open", "reef_merkle_read_level", "reef_merkle_check_paths"}
    assert new <= names, new - names
    assert "reef_merkle_ctx" in open(_ffi.HEADER).read()                  # the seventh new name is the opaque type
    lib = _ffi.load()
    assert all(getattr(lib, n).argtypes is not None for n in new)
    assert lib.reef_abi_version() == 7                                    # symbols are added, none changed
