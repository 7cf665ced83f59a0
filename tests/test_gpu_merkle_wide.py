"""Row N4 where the other Merkle tests do not reach: the thread-per-node kernels (k_pos_leaves, k_pos_nodes, k_pos_paths_wide and the per-thread
poseidon_permute_sparse / _dense of merkle_kernels.inc), which hash every level above POS_SPREAD_MAX_NODES = 16384 nodes; the Montgomery form
and device buffers of the one-shot calls; constants and inputs at the extremes of the lazy dot products.  Every comparison is bit for bit with
oracle.merkle_oracle (the permutation as defined, in Python integers, ~1 ms a hash: big trees are sampled, small ones compared whole).

Three parts.  The release build at the shipped threshold (sampled).  The experiment build in a child process with the five-lane form switched
off, or handed over at 64 nodes, so that small trees go node for node through the thread-per-node kernels: one child per switch setting, started
by the first test that needs it, its outcome kept for the others (a child that ended abnormally, ran into its time limit or could not be
started fails them all and is not started again).  The release build again for Montgomery form, device buffers, argument errors and extreme
constants."""
import numpy as np
import pytest

from merkle_drivers import (DEVICE, RESIDENT_CHECKS, case_key, commit_call, commit_raw, expected_open, first_mismatch, make_doc, make_params,
                            oracle_case, oracle_tree, path_alterations, run_child, tree_case)
from oracle import merkle_oracle as M

pytestmark = pytest.mark.gpu

CURVES = ["pallas", "vesta"]


def leaf_hash(doc, i, p):
    right = [2 * i + 1, doc[2 * i + 1]] if 2 * i + 1 < len(doc) else [0, 0]
    return M.hash_query([2 * i, doc[2 * i]] + right, p)


def node_hash(below, i, p):
    return M.hash_query([below[2 * i], below[2 * i + 1] if 2 * i + 1 < len(below) else 0], p)


# ---------------------------------------------------------------------------------- 1. the shipped threshold, release build ----

def check_sampled_tree(curve, n, doc, p, root, tree, fixed, n_random, upper_samples):
    """Level 0 at `fixed` and n_random seeded nodes against the oracle's hash of the document; level h in upper_samples = {h: (fixed, n_random)}
    against the oracle's hash of the GPU's own children; every node of every level of at most 1024 nodes against the level below."""
    rng = np.random.default_rng(n)
    sizes = [len(lv) for lv in tree]
    want_sizes = [(n + 1) // 2]
    while want_sizes[-1] > 1:
        want_sizes.append((want_sizes[-1] + 1) // 2)
    assert sizes == want_sizes
    for i in sorted(set(fixed) | {int(x) for x in rng.integers(0, sizes[0], size=n_random)}):
        assert tree[0][i] == leaf_hash(doc, i, p), (curve, n, 0, i)
    for h, (fix, k) in upper_samples.items():
        for i in sorted(set(fix) | {int(x) for x in rng.integers(0, sizes[h], size=k)}):
            assert tree[h][i] == node_hash(tree[h - 1], i, p), (curve, n, h, i)
    for h in range(1, len(tree)):
        if sizes[h] <= 1024:
            for i in range(sizes[h]):
                assert tree[h][i] == node_hash(tree[h - 1], i, p), (curve, n, h, i)
    assert root == tree[-1][0]


def test_both_forms_at_the_threshold_65537(gpu_lib):
    """32769 leaf nodes (k_pos_leaves, the last a lone symbol), 16385 above (k_pos_nodes, the last with no right child), then 8193: the first
    five-lane level, which reads what k_pos_nodes wrote."""
    n, p = 65537, make_params("pallas")
    doc = make_doc(n, "edge")
    root, tree = commit_raw("pallas", doc, p, False)
    assert [len(lv) for lv in tree[:3]] == [32769, 16385, 8193]
    check_sampled_tree("pallas", n, doc, p, root, tree, [0, 1, 255, 256, 257, 32767, 32768], 40,
                       {1: ([0, 1, 255, 256, 16383, 16384], 40), 2: ([0, 8192], 20)})


@pytest.mark.parametrize("n", [32768, 32770])
def test_leaf_level_either_side_of_the_threshold(n, gpu_lib):
    """16384 leaf nodes: the last size the five-lane form takes; 16385: the first it does not.  Vesta's field, canonical form."""
    p = make_params("vesta")
    doc = make_doc(n, "edge")
    root, tree = commit_raw("vesta", doc, p, False)
    m0 = (n + 1) // 2
    assert len(tree[0]) == m0 == {32768: 16384, 32770: 16385}[n]
    check_sampled_tree("vesta", n, doc, p, root, tree, [0, 11, 12, 255, 256, m0 - 1], 30, {})


# ------------------------------------------------------------ 2. a thread per node everywhere: the experiment build in a child ----

TREE_SIZES = [1, 2, 3, 4, 7, 8, 511, 512, 513, 514, 1001]
SWEEP = [(8, rp) for rp in (0, 1, 2, 7, 8, 9, 16, 17, 57)] + [(2, 9)]
RESIDENT = {"op": "resident", "curve": "vesta", "n": 1001}
CASES = {
    "thread_per_node": [tree_case(c, n) for c in CURVES for n in TREE_SIZES]                       # Pallas canonical, Vesta Montgomery
                       + [tree_case(c, 21, rf=rf, rp=rp) for c in CURVES for rf, rp in SWEEP]
                       + [tree_case(c, 513, "ext", kind) for c in CURVES for kind in ("mixed", "all_max")]
                       + [tree_case(c, 21, pkind="cycled", rp=1024) for c in CURVES]
                       + [RESIDENT],
    "thread_per_node_dense": [tree_case(c, n, rp=rp) for c in CURVES for n in (3, 513) for rp in (0, 9, 56)],
    "hand_over_at_64": [tree_case(c, n) for c in CURVES for n in (129, 1001)],
}


_children = {}


def child(setting):
    """The outcome of the one child of this setting, whatever it was: a child is started once per session, also when starting it raised."""
    if setting not in _children:
        try:
            _children[setting] = run_child(setting, CASES[setting])
        except Exception as e:                                                 # noqa: BLE001 -- kept, so that no later test starts it again
            _children[setting] = (-1, {}, f"{type(e).__name__}: {e}")
    return _children[setting]


def child_out(setting, case):
    code, outs, err = child(setting)
    assert code == 0, (setting, code, err)
    assert case_key(case) in outs, (setting, case)
    return outs[case_key(case)]


def check_child_tree(setting, case):
    got = child_out(setting, case)
    _, root, tree = oracle_case(case["curve"], case["n"], case["doc"], case["pkind"], case["rf"], case["rp"])
    got_tree = [[int(x, 16) for x in lv] for lv in got["tree"]]
    assert first_mismatch(got_tree, tree) is None, (case["curve"], case["n"], case["rf"], case["rp"], case["pkind"]) + tuple(first_mismatch(got_tree, tree))
    assert int(got["root"], 16) == root


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", TREE_SIZES)
def test_thread_per_node_whole_trees(n, curve, gpu_lib):
    """REEF_POSEIDON_SPREAD=0: k_pos_leaves and k_pos_nodes hash every level.  256 and 257 leaf nodes (a second block with one live thread), a lone
    last symbol, an odd node count at some level of every size."""
    check_child_tree("thread_per_node", tree_case(curve, n))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("rf,rp", SWEEP)
def test_thread_per_node_partial_round_sweep(rf, rp, curve, gpu_lib):
    """The per-thread sparse round around its renormalisation every 8 rounds, and with a single full round either side."""
    check_child_tree("thread_per_node", tree_case(curve, 21, rf=rf, rp=rp))


@pytest.mark.parametrize("curve", CURVES)
def test_thread_per_node_most_partial_rounds(curve, gpu_lib):
    """1024 partial rounds, the most the library takes: 1023 sparse rounds from a table of 10230 derived constants, 127 renormalisations."""
    check_child_tree("thread_per_node", tree_case(curve, 21, pkind="cycled", rp=1024))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["mixed", "all_max"])
def test_thread_per_node_extreme_constants(kind, curve, gpu_lib):
    """The extremes of part 4 through the per-thread kernels, across a block boundary."""
    check_child_tree("thread_per_node", tree_case(curve, 513, "ext", kind))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [3, 513])
@pytest.mark.parametrize("rp", [0, 9, 56])
def test_thread_per_node_dense_rounds(rp, n, curve, gpu_lib):
    """REEF_POSEIDON_DENSE=1 as well: poseidon_permute_dense through k_pos_leaves / k_pos_nodes."""
    check_child_tree("thread_per_node_dense", tree_case(curve, n, rp=rp))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [129, 1001])
def test_hand_over_between_the_two_forms(n, curve, gpu_lib):
    """REEF_POSEIDON_SPREAD_MAX=64: levels of 501, 251, 126 (or 65) nodes a thread per node, 63 (33) and below five lanes per hash -- one form
    writes the level the other reads."""
    check_child_tree("hand_over_at_64", tree_case(curve, n))


def test_thread_per_node_resident_tree_in_montgomery_form(gpu_lib):
    """The resident tree on Vesta with the five-lane form off: every opening, and reef_merkle_check_paths through k_pos_paths_wide whatever the
    number of paths -- honest openings accepted, each alteration of one opening rejecting that one alone."""
    got = child_out("thread_per_node", RESIDENT)
    doc, root, tree = oracle_tree("vesta", 1001)
    n, L = len(doc), len(tree)
    esym, eoidx, eopp, epath = expected_open(doc, tree, list(range(n)))
    assert (int(got["root"], 16), got["levels"]) == (root, L)
    assert got["sym"] == esym and got["oidx"] == eoidx
    assert [int(x, 16) for x in got["opp"]] == eopp
    assert [int(x, 16) for x in got["path"]] == epath
    assert [(c["k"], c["victim"]) for c in got["checks"]] == list(RESIDENT_CHECKS)
    for c in got["checks"]:
        k, victim = c["k"], c["victim"]
        assert [(name, depth) for name, depth, _ in c["runs"]] == [("honest", None)] + path_alterations(L)
        for name, depth, accept in c["runs"]:
            want = [1] * k if name == "honest" else [0 if j == victim else 1 for j in range(k)]
            assert accept == want, (k, victim, name, depth)


# ------------------------------------------------------------------------ 3. Montgomery form and device buffers, release build ----

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 100, 1001])
def test_one_shot_commit_in_montgomery_form(n, curve, gpu_lib):
    doc, root, tree = oracle_case(curve, n)
    got_root, got_tree = commit_raw(curve, doc, make_params(curve), True)
    assert first_mismatch(got_tree, tree) is None, (curve, n, first_mismatch(got_tree, tree))
    assert got_root == root


@pytest.mark.parametrize("curve", CURVES)
def test_alternating_forms_and_tags_in_one_process(curve, gpu_lib):
    """The derived constants are kept for the last parameter set (its form included); the tags are not part of that key and are imported per call."""
    n, p = 100, make_params(curve)
    doc, root, tree = oracle_case(curve, n)
    for mont in (False, True, False):
        assert commit_raw(curve, doc, p, mont) == (root, tree), mont
    p2 = M.Params(p.m, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf + 1, p.m - 1)
    want = M.commit(doc, p2)
    assert want[0] != root
    for mont in (False, True):
        assert commit_raw(curve, doc, p2, mont) == want, mont
    assert commit_raw(curve, doc, p, True) == (root, tree)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [3, 9, 33, 257, 1001])
def test_commit_in_blocks_in_montgomery_form(n, curve, gpu_lib):
    """reef_merkle_commit_devices with three members: one block (n = 3), several, and the blocks' roots imported for the levels above."""
    doc, root, tree = oracle_case(curve, n)
    p = make_params(curve)
    got_root, got_tree = commit_raw(curve, doc, p, True, devices=[0, 0, 0])
    assert first_mismatch(got_tree, tree) is None, (curve, n, first_mismatch(got_tree, tree))
    assert got_root == root
    assert commit_raw(curve, doc, p, True, devices=[0, 0, 0], want_tree=False) == (root, [])


@pytest.mark.parametrize("mont", [False, True])
def test_device_document_and_device_tree(mont, gpu_lib):
    doc, root, tree = oracle_case("pallas", 1001)
    p = make_params("pallas")
    host = commit_raw("pallas", doc, p, mont)
    assert commit_raw("pallas", doc, p, mont, doc_loc=DEVICE, tree_loc=DEVICE) == host
    assert host == (root, tree)


@pytest.mark.parametrize("what,header,n,message", [("rf=0", (5, 0, 56), 8, "round numbers"), ("rf=66", (5, 66, 56), 8, "round numbers"), ("rp=1025", (5, 8, 1025), 8, "round numbers"),
                                                   ("width=4", (4, 8, 56), 8, "width 4"), ("n=0", (5, 8, 56), 0, "document length")])
def test_argument_errors_leave_the_outputs_alone(what, header, n, message, gpu_lib):
    fill = 0xA5A5A5A5A5A5A5A5
    p = make_params("pallas")
    assert commit_call("pallas", [1, 2], p, False, header=(3, 8, 56) if what != "width=4" else (5, 0, 56))[0] == 1    # another error's message is the last one now
    assert message not in gpu_lib.reef_last_error().decode()
    st, tree, root = commit_call("pallas", make_doc(n, "lin"), p, False, fill=fill, header=header)
    assert st == 1, what                                                      # REEF_ERR_ARG
    assert message in gpu_lib.reef_last_error().decode(), (what, gpu_lib.reef_last_error().decode())
    assert (tree == fill).all() and (root == fill).all(), what


# ------------------------------------------------------------------------------ 4. constants and inputs at the extremes ----

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["mixed", "all_max", "singular_block"])
@pytest.mark.parametrize("mont", [False, True])
def test_extreme_constants_and_symbols(mont, kind, curve, gpu_lib):
    """mixed takes the sparse form; all_max and singular_block have a singular lower-right block, so the release build falls back to the dense
    rounds (tests/test_merkle_inputs_host.py states what these inputs are)."""
    for n, rp in [(1, 56), (2, 56), (7, 56), (100, 56), (257, 56), (21, 9), (21, 57)]:
        doc, root, tree = oracle_case(curve, n, "ext", kind, 8, rp)
        got_root, got_tree = commit_raw(curve, doc, make_params(curve, kind, 8, rp), mont)
        assert first_mismatch(got_tree, tree) is None, (curve, kind, mont, n, rp, first_mismatch(got_tree, tree))
        assert got_root == root
