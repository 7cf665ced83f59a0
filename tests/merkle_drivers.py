"""What the Poseidon Merkle tests (row N4) share: the oracle's trees, computed once per case, the C ABI driven directly with field elements
in either form, the constants at their extremes, and a child process that runs cases on the experiment build under a switch.

Run as a program (`python tests/merkle_drivers.py '<json list of cases>'`) this is the child: it makes the GPU calls of every case on whatever
library REEF_MSM_LIB names, prints one JSON line per case and exits non-zero on a ReefError.  The parent (run_child) compares."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import merkle_oracle as M  # noqa: E402

FIELDS = {"pallas": (M.Q, False), "vesta": (M.P, True)}      # curve -> (its scalar field, the form the test hands field elements over in)
R = 1 << 256
HOST, DEVICE = 0, 1


@functools.lru_cache(maxsize=None)
def params(curve):
    return M.standin_params(FIELDS[curve][0])


@functools.lru_cache(maxsize=None)
def oracle_tree(curve, n, mul=31, add=7):
    doc = [(mul * i + add) % 131 for i in range(n)]
    root, tree = M.commit(doc, params(curve))
    return doc, root, tree


def limbs(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def table_max(mod):
    """The integer whose internal form x * 2^261 mod M is 2^254 - 1: limbs 0..7 at 2^29 - 1, the top limb at 2^22 - 1."""
    return ((1 << 254) - 1) * pow(2, -261, mod) % mod


def extreme_params(mod, kind, rf=8, rp=56):
    """Poseidon parameters whose matrix operands sit where the lazy dot products (fe_vec.h: wide18_mac, four products between carries) are
    tightest.  mixed: M - 1, table max, 0, 1, M - 2, table max + 1 through the matrix, the round constants and the tags, with the matrix and
    its lower-right 4 x 4 block regular (the sparse form is taken).  all_max: every matrix entry and tag the table max, every round constant
    M - 1; the block is singular, so the library falls back to the dense rounds.  singular_block: the stand-ins with row 2 of the block
    a copy of row 1 -- the same fallback on ordinary values."""
    t = table_max(mod)
    if kind == "mixed":
        ext = [mod - 1, t, 0, 1, mod - 2, t + 1]
        mds = [[ext[(i * i + 3 * j + i * j) % 6] for j in range(5)] for i in range(5)]
        return M.Params(mod, 5, rf, rp, [ext[k % 6] for k in range(5 * (rf + rp))], mds, mod - 1, t)
    if kind == "all_max":
        return M.Params(mod, 5, rf, rp, [mod - 1] * (5 * (rf + rp)), [[t] * 5 for _ in range(5)], t, t)
    if kind == "singular_block":
        p = M.standin_params(mod, 5, rf, rp)
        p.mds[2][1:] = p.mds[1][1:]
        return p
    raise ValueError(kind)


# ---- cases: (curve, n, doc kind, parameter kind, rf, rp), everything the oracle's tree depends on ----

def make_doc(n, dockind):
    if dockind == "lin":
        return [(31 * i + 7) % 131 for i in range(n)]
    if dockind == "edge":                                     # 32-bit symbols at both ends
        doc = [(31 * i + 7) % 131 for i in range(n)]
        doc[0] = doc[-1] = 0xFFFFFFFF
        return doc
    if dockind == "ext":
        return [(0, 1, 0xFFFFFFFF, 0xFFFFFFFE)[i % 4] for i in range(n)]
    raise ValueError(dockind)


@functools.lru_cache(maxsize=None)
def make_params(curve, pkind="standin", rf=8, rp=56):
    mod = FIELDS[curve][0]
    if pkind == "standin":
        return M.standin_params(mod, 5, rf, rp)
    if pkind == "cycled":                                     # the stand-ins of 8 + 56 rounds, their round constants repeated: long runs of rounds at no cost
        base = M.standin_params(mod)
        return M.Params(mod, 5, rf, rp, [base.rc[k % len(base.rc)] for k in range(5 * (rf + rp))], base.mds, base.tag_leaf, base.tag_node)
    return extreme_params(mod, pkind, rf, rp)


@functools.lru_cache(maxsize=None)
def oracle_case(curve, n, dockind="lin", pkind="standin", rf=8, rp=56):
    """-> (doc, root, tree) of the oracle, once per case"""
    doc = make_doc(n, dockind)
    root, tree = M.commit(doc, make_params(curve, pkind, rf, rp))
    return doc, root, tree


def first_mismatch(got, want):
    """(level, node) of the first node at which two trees differ, or a word on their shapes; None when they are the same tree"""
    if [len(lv) for lv in got] != [len(lv) for lv in want]:
        return "level sizes", [len(lv) for lv in got], [len(lv) for lv in want]
    for h, (a, b) in enumerate(zip(got, want)):
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return h, i
    return None


def det(rows, mod):
    """Determinant of a square matrix over the field (Gaussian elimination)."""
    a, d = [list(r) for r in rows], 1
    for c in range(len(a)):
        piv = next((r for r in range(c, len(a)) if a[r][c] % mod), None)
        if piv is None:
            return 0
        if piv != c:
            a[piv], a[c], d = a[c], a[piv], -d
        d = d * a[c][c] % mod
        inv = pow(a[c][c], -1, mod)
        for r in range(c + 1, len(a)):
            f = a[r][c] * inv % mod
            a[r] = [(x - f * y) % mod for x, y in zip(a[r], a[c])]
    return d % mod


# ---- the C ABI itself ----

def _form(x, mod, mont):
    return x * R % mod if mont else x


def _fe_array(xs, mod, mont):
    return np.array([limbs(_form(x, mod, mont)) for x in xs], dtype=np.uint64).reshape(-1, 4)


def _ints(arr, mod, mont):
    out = [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in arr]
    if mont:
        rinv = pow(R, -1, mod)
        out = [x * rinv % mod for x in out]
    return out


def level_sizes(n):
    sizes, m = [], (n + 1) // 2
    while True:
        sizes.append(m)
        if m <= 1:
            return sizes
        m = (m + 1) // 2


def commit_call(curve, doc, p, is_mont, devices=None, doc_loc=HOST, tree_loc=HOST, want_tree=True, fill=0, header=None):
    """One reef_merkle_commit (devices None) or reef_merkle_commit_devices, the arguments as the C caller lays them out.
    -> (status, tree limbs, root limbs): the two host outputs start as `fill`, so that an untouched one shows.  header: (width, rf, rp) to
    put in the struct in place of the parameters' own (the constant arrays are stretched to what the header asks for).  With doc_loc / tree_loc
    DEVICE the document goes up into a DeviceBuffer and the tree comes back from a second one."""
    from reef_amd import _ffi, merkle, msm
    lib, mod = _ffi.load(), FIELDS[curve][0]
    width, rf, rp = header or (p.t, p.rf, p.rp)
    need = max(len(p.rc), 5 * (rf + rp), 1)
    rc = _fe_array([p.rc[k % len(p.rc)] for k in range(need)], mod, is_mont)
    mds = _fe_array([x for row in p.mds for x in row], mod, is_mont)
    pp = merkle.PoseidonParams(width, rf, rp, 0, rc.ctypes.data, mds.ctypes.data, (ctypes.c_uint64 * 4)(*limbs(_form(p.tag_leaf, mod, is_mont))),
                               (ctypes.c_uint64 * 4)(*limbs(_form(p.tag_node, mod, is_mont))))
    d = np.ascontiguousarray(np.asarray(doc, dtype=np.uint32))
    n = d.shape[0]
    total = sum(level_sizes(n)) if n else 1
    tree = np.full((total, 4), fill, dtype=np.uint64)
    root = np.full((1, 4), fill, dtype=np.uint64)
    keep = []
    try:
        d_ptr, t_ptr = d.ctypes.data, tree.ctypes.data if want_tree else None
        if doc_loc == DEVICE:
            keep.append(msm.DeviceBuffer.from_host(d))
            d_ptr = keep[-1].ptr
        if tree_loc == DEVICE and want_tree:
            keep.append(msm.DeviceBuffer.from_host(tree))
            t_ptr = keep[-1].ptr
        if devices is None:
            st = lib.reef_merkle_commit(msm.curve_id(curve), ctypes.byref(pp), d_ptr, n, doc_loc, is_mont, t_ptr, tree_loc, root.ctypes.data)
        else:
            assert doc_loc == HOST and tree_loc == HOST
            devs = (ctypes.c_int * len(devices))(*devices)
            st = lib.reef_merkle_commit_devices(msm.curve_id(curve), ctypes.byref(pp), d_ptr, n, is_mont, devs, len(devices), t_ptr, root.ctypes.data, None)
        if st == 0 and tree_loc == DEVICE and want_tree:
            _ffi.check(lib.reef_device_sync())
            tree = keep[-1].to_host(tree.shape)
    finally:
        for b in keep:
            b.free()
    return st, tree, root


def commit_raw(curve, doc, p, is_mont, devices=None, doc_loc=HOST, tree_loc=HOST, want_tree=True):
    """-> (root, levels) as integers, whichever form crossed the ABI (x * 2^256 mod m is the Montgomery form, converted here); levels is empty
    when want_tree is False (tree_out = NULL).  Raises ReefError."""
    from reef_amd import _ffi
    st, tree, root = commit_call(curve, doc, p, is_mont, devices, doc_loc, tree_loc, want_tree)
    _ffi.check(st)
    mod = FIELDS[curve][0]
    levels, off = [], 0
    if want_tree:
        flat = _ints(tree, mod, is_mont)
        for m in level_sizes(len(doc)):
            levels.append(flat[off:off + m])
            off += m
    return _ints(root, mod, is_mont)[0], levels


class Raw:
    """The C ABI itself, field elements in either form: Python integers in and out, converted here (x * 2^256 mod m is the Montgomery form)."""

    def __init__(self, curve, doc, device=0):
        from reef_amd import _ffi, merkle, msm
        self.lib, self.m, self.mont = _ffi.load(), FIELDS[curve][0], FIELDS[curve][1]
        self.rinv = pow(R, -1, self.m)
        p = params(curve)
        self._rc, self._mds = self.fe_array(p.rc), self.fe_array([x for row in p.mds for x in row])
        pp = merkle.PoseidonParams(p.t, p.rf, p.rp, 0, self._rc.ctypes.data, self._mds.ctypes.data, (ctypes.c_uint64 * 4)(*limbs(self.to_form(p.tag_leaf))),
                                   (ctypes.c_uint64 * 4)(*limbs(self.to_form(p.tag_node))))
        d = np.ascontiguousarray(np.asarray(doc, dtype=np.uint32))
        self.h = ctypes.c_void_p()
        _ffi.check(self.lib.reef_merkle_create(ctypes.byref(self.h), msm.curve_id(curve), ctypes.byref(pp), d.ctypes.data, d.shape[0], 0, self.mont, device))
        n, lv, nodes = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        root = np.zeros((1, 4), dtype=np.uint64)
        _ffi.check(self.lib.reef_merkle_info(self.h, ctypes.byref(n), ctypes.byref(lv), ctypes.byref(nodes), root.ctypes.data))
        self.n, self.levels, self.nodes, self.root = n.value, lv.value, nodes.value, self.ints(root)[0]

    def to_form(self, x):
        return x * R % self.m if self.mont else x

    def fe_array(self, xs):
        return np.array([limbs(self.to_form(x)) for x in xs], dtype=np.uint64).reshape(-1, 4)

    def ints(self, arr):
        out = [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in arr]
        return [x * self.rinv % self.m for x in out] if self.mont else out

    def open(self, idx, want_sym=True, want_oidx=True, want_path=True, fill=0):
        """-> (status, symbols, opposite_idx, opposite ints, path ints); outputs start as `fill` so that an untouched one shows"""
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
        k, L = idx.shape[0], self.levels
        sym = np.full(max(k, 1), fill, dtype=np.uint32)
        oidx = np.full(max(k, 1), fill, dtype=np.uint64)
        opp = np.full((max(k * L, 1), 4), fill, dtype=np.uint64)
        path = np.full((max(k * L, 1), 4), fill, dtype=np.uint64)
        st = self.lib.reef_merkle_open(self.h, idx.ctypes.data, k, sym.ctypes.data if want_sym else None, oidx.ctypes.data if want_oidx else None, opp.ctypes.data,
                                       path.ctypes.data if want_path else None)
        self.raw_out = (sym, oidx, opp, path)
        return st, sym[:k].tolist(), oidx[:k].tolist(), self.ints(opp[:k * L]), self.ints(path[:k * L])

    def read_level(self, level, first, count):
        out = np.zeros((max(count, 1), 4), dtype=np.uint64)
        st = self.lib.reef_merkle_read_level(self.h, level, first, count, out.ctypes.data, 0)
        return st, self.ints(out[:count])

    def check_paths(self, idx, sym, oidx, opp, raw_opp=None):
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
        sym = np.ascontiguousarray(np.asarray(sym, dtype=np.uint32))
        oidx = np.ascontiguousarray(np.asarray(oidx, dtype=np.uint64))
        o = raw_opp if raw_opp is not None else self.fe_array(opp)
        accept = np.full(max(idx.shape[0], 1), 7, dtype=np.uint32)
        st = self.lib.reef_merkle_check_paths(self.h, idx.ctypes.data, sym.ctypes.data, oidx.ctypes.data, o.ctypes.data, idx.shape[0], accept.ctypes.data)
        return st, accept[:idx.shape[0]].tolist()

    def error(self):
        return self.lib.reef_last_error().decode()

    def close(self):
        if self.h:
            self.lib.reef_merkle_destroy(self.h)
            self.h = None


def expected_open(doc, tree, idx):
    """reef_merkle_open's arrays from the oracle's tree: (symbols, opposite_idx, opposite, path), the last two query-major."""
    n, L = len(doc), len(tree)
    sym, oidx, opp, path = [], [], [], []
    for q in idx:
        sib = q ^ 1
        sym.append(doc[q])
        oidx.append(sib if sib < n else 0)
        opp.append(doc[sib] if sib < n else 0)
        for h in range(L - 1):
            s = (q >> (h + 1)) ^ 1
            opp.append(tree[h][s] if s < len(tree[h]) else 0)
        path += [tree[h][q >> (h + 1)] for h in range(L)]
    return sym, oidx, opp, path


def path_alterations(L):
    """(field, depth) of what the check of one opening must notice: the symbol, the sibling's index, the sibling at the bottom, the middle and the top"""
    return [("symbols", None), ("opposite_idx", None)] + [("opposite", d) for d in sorted({0, L // 2, L - 1})]


RESIDENT_CHECKS = ((13, 5), (700, 699))           # (paths in the call, the altered one): inside the first block, the last thread of the third


# ---- the child: the experiment build under a switch, one process for all the cases of that switch ----

def tree_case(curve, n, dockind="lin", pkind="standin", rf=8, rp=56, mont=None):
    return {"op": "commit", "curve": curve, "n": n, "doc": dockind, "pkind": pkind, "rf": rf, "rp": rp, "mont": FIELDS[curve][1] if mont is None else mont}


def case_key(c):
    return json.dumps(c, sort_keys=True)


def _hexes(xs):
    return [format(x, "x") for x in xs]


def _run_case(c):
    if c["op"] == "commit":
        root, levels = commit_raw(c["curve"], make_doc(c["n"], c["doc"]), make_params(c["curve"], c["pkind"], c["rf"], c["rp"]), c["mont"])
        return {"root": format(root, "x"), "tree": [_hexes(lv) for lv in levels]}
    assert c["op"] == "resident"
    doc, _, tree = oracle_tree(c["curve"], c["n"])            # the honest openings the check is given are the oracle's, not the tree's own
    n, L = len(doc), len(tree)
    t = Raw(c["curve"], doc)
    try:
        st, sym, oidx, opp, path = t.open(list(range(n)))
        if st:
            raise RuntimeError(t.error())
        out = {"root": format(t.root, "x"), "levels": t.levels, "sym": sym, "oidx": oidx, "opp": _hexes(opp), "path": _hexes(path), "checks": []}
        for k, victim in RESIDENT_CHECKS:
            idx = [(5 * j + 3) % n for j in range(k)]
            esym, eoidx, eopp, _ = expected_open(doc, tree, idx)
            runs = []
            for name, depth in [("honest", None)] + path_alterations(L):
                s2, o2, p2 = list(esym), list(eoidx), list(eopp)
                if name == "symbols":
                    s2[victim] += 1
                elif name == "opposite_idx":
                    o2[victim] += 1
                elif name == "opposite":
                    p2[victim * L + depth] = (p2[victim * L + depth] + 1) % t.m
                st, accept = t.check_paths(idx, s2, o2, p2)
                if st:
                    raise RuntimeError(t.error())
                runs.append([name, depth, accept])
            out["checks"].append({"k": k, "victim": victim, "runs": runs})
        return out
    finally:
        t.close()


def child_main(argv):
    from reef_amd import _ffi
    try:
        for c in json.loads(argv[1]):
            print(json.dumps({"case": case_key(c), "out": _run_case(c)}), flush=True)
    except (_ffi.ReefError, RuntimeError) as e:
        print(f"child: {e}", file=sys.stderr)
        return 3
    return 0


SWITCHES = {                                                  # the experiment build's switches, read once per process (common.h: exp_env)
    "thread_per_node": {"REEF_POSEIDON_SPREAD": "0"},
    "thread_per_node_dense": {"REEF_POSEIDON_SPREAD": "0", "REEF_POSEIDON_DENSE": "1"},
    "hand_over_at_64": {"REEF_POSEIDON_SPREAD_MAX": "64"},
}


def run_child(setting, cases, timeout=300):
    """-> (return code, {case_key: out}, the end of stderr): a fresh python on the experiment build with the switches of `setting`.  A child that
    does not end within `timeout` is killed and reported as return code 124, as `timeout` does: an outcome like any other, not an exception."""
    from reef_amd import _ffi
    env = dict(os.environ, REEF_MSM_LIB=_ffi.EXPERIMENT_LIB_PATH, **SWITCHES[setting])
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(cases)], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
        code, stdout, stderr = run.returncode, run.stdout, run.stderr
    except subprocess.TimeoutExpired as e:
        text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")      # noqa: E731
        code, stdout, stderr = 124, "", f"no end within {timeout} s; " + text(e.stderr)
    outs = {}
    for line in stdout.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            outs[rec["case"]] = rec["out"]
    return code, outs, stderr[-2000:]


if __name__ == "__main__":
    sys.exit(child_main(sys.argv))
