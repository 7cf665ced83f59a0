"""INTEGRATION.md shows the bindings a Reef / nova-snark maintainer would add (`extern "C"` blocks, `#[repr(C)]` structs).  They are
the reference-side half of the drop-in boundary (include/reef_msm.h), so they must not drift from the header: every Rust declaration
is parsed and compared with the C prototype of the same name -- number of arguments, pointer / integer / bool kinds and widths, the
return type -- and every `#[repr(C)]` struct with the header's struct, field for field."""
import os
import re

from abi_text import ROOT, header_prototypes, rust_kind, split_top, strip_comments


def test_every_rust_declaration_matches_the_header():
    protos = header_prototypes()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    seen = 0
    for m in re.finditer(r"\bfn\s+((?:reef_|mult_pippenger_)\w+)\s*\(([^;{}]*?)\)\s*(?:->\s*([^;{]+?))?\s*;", doc, flags=re.S):
        name, args, ret = m.group(1), strip_comments(m.group(2)), (m.group(3) or "void").strip()
        assert name in protos, f"INTEGRATION.md binds {name}, which include/reef_msm.h does not declare"
        got = (rust_kind(ret), [rust_kind(a.split(":", 1)[1]) for a in split_top(args)])
        assert got == protos[name], f"{name}: INTEGRATION.md declares {got}, the header {protos[name]}"
        seen += 1
    assert seen >= 20            # the drop-in pair, the handle API, device groups, sum-check, document polynomial, Merkle, key derivation


def _c_struct_fields(name):
    hdr = strip_comments(open(os.path.join(ROOT, "include", "reef_msm.h")).read())
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*" + name + r"\s*;", hdr).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = decl.rsplit(" ", 1)[0] if "," not in decl else decl.split(",")[0].rsplit(" ", 1)[0]
        for part in decl[len(ctype):].split(","):
            fields.append(re.sub(r"[\*\s]|\[.*?\]", "", part))
    return fields


def test_repr_c_structs_list_the_header_fields_in_order():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    pairs = {"ReefMsmOpts": "reef_msm_opts", "ReefGroupOpts": "reef_msm_group_opts", "ReefPoseidonParams": "reef_poseidon_params",
             "ReefKeygenParams": "reef_keygen_params"}
    for rust, c in pairs.items():
        body = re.search(r"#\[repr\(C\)\]\s*(?:pub\s+)?struct\s+" + rust + r"\s*\{(.*?)\}", doc, flags=re.S).group(1)
        names = [f.split(":")[0].strip() for f in split_top(strip_comments(body))]
        assert names == _c_struct_fields(c), f"{rust}: {names} against {c}: {_c_struct_fields(c)}"


def test_the_ctypes_binding_matches_the_header():
    """reef_amd/_ffi.py is how every GPU test, the soak and bench.py reach the library: an argument of the wrong width there would be a bug
    in the checker, not in the product.  Every function the binding declares is compared with the header's prototype."""
    import ctypes

    from reef_amd import _ffi
    lib = _ffi.load()                                    # loads without a GPU (tests/test_abi.py)
    protos = header_prototypes()

    def kind(t):
        if t is None:
            return "void"
        if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents"):
            return "ptr"
        return {ctypes.c_int: "i32", ctypes.c_uint32: "u32", ctypes.c_uint64: "u64", ctypes.c_bool: "bool"}[t]   # c_size_t IS c_uint64 here
    bound = 0
    for name, (ret_, args_) in protos.items():
        want = (ret_.replace("usize", "u64"), [a.replace("usize", "u64") for a in args_])
        fn = getattr(lib, name)
        if fn.argtypes is None:
            continue                                     # declared in the header, not used from Python
        got = (kind(fn.restype), [kind(t) for t in fn.argtypes])
        assert got == want, f"{name}: _ffi.py declares {got}, the header {want}"
        bound += 1
    assert bound >= 60
