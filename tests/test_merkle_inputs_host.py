"""What the extreme Poseidon inputs of tests/test_gpu_merkle_wide.py are (merkle_drivers.extreme_params), stated on the host: which of them
take the sparse form of the partial rounds and which the dense fallback.  The library derives the sparse constants by inverting the lower-right
4 x 4 block of M_k, and that block of M_k is D_0^(k+1) for D_0 the block of the caller's matrix (the lower-right block of diag(1, D) * M is
D * D_0): the derivation fails exactly when D_0 is singular."""
import pytest

from merkle_drivers import FIELDS, det, extreme_params, first_mismatch, make_params, oracle_case, table_max
from oracle import merkle_oracle as M


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_table_max_is_the_largest_internal_form(curve):
    mod = FIELDS[curve][0]
    t = table_max(mod)
    assert 0 < t < mod - 2 and t * (1 << 261) % mod == (1 << 254) - 1


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_which_inputs_take_the_sparse_form(curve):
    mod = FIELDS[curve][0]
    block = lambda p: [row[1:] for row in p.mds[1:]]                          # noqa: E731
    mixed, all_max, singular = (extreme_params(mod, kind) for kind in ("mixed", "all_max", "singular_block"))
    assert det(mixed.mds, mod) != 0 and det(block(mixed), mod) != 0
    assert det(block(all_max), mod) == 0 and det(all_max.mds, mod) == 0
    assert det(block(singular), mod) == 0
    standin = M.standin_params(mod)
    assert det(standin.mds, mod) != 0 and det(block(standin), mod) != 0      # the stand-ins themselves are regular
    assert singular.mds[2][0] == standin.mds[2][0] and singular.mds[2][1:] == standin.mds[1][1:]
    ext = {mod - 1, table_max(mod), 0, 1, mod - 2, table_max(mod) + 1}
    assert {x for row in mixed.mds for x in row} == ext and set(mixed.rc) == ext and len(mixed.rc) == 5 * (8 + 56)
    assert (mixed.tag_leaf, mixed.tag_node) == (mod - 1, table_max(mod))
    assert {x for row in all_max.mds for x in row} == {table_max(mod)} and set(all_max.rc) == {mod - 1}
    assert det([[2, 1], [1, 1]], mod) == 1 and det([[0, 1], [1, 0]], mod) == mod - 1 and det([[1, 2], [2, 4]], mod) == 0


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_the_singular_block_reaches_the_digest(curve):
    n = 7
    doc, root, tree = oracle_case(curve, n, "ext", "singular_block")
    root0, tree0 = M.commit(doc, make_params(curve))
    assert root != root0 and first_mismatch(tree, tree0) == (0, 0)
