"""The text side of the ABI checks: include/reef_msm.h's prototypes and INTEGRATION.md's Rust declarations reduced to the same kinds
(pointer / integer / bool and widths).  Shared by tests/test_integration_doc.py and tests/test_hyrax_eval_host.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_KINDS = {"size_t": "usize", "int": "i32", "int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "uint8_t": "u8", "bool": "bool",
           "reef_status": "i32", "void": "void"}


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def split_top(args):
    parts, depth, cur = [], 0, ""
    for ch in args:
        depth += ch in "[(<"
        depth -= ch in "])>"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return [p for p in parts + [cur] if p.strip()]


def header_prototypes():
    hdr = strip_comments(open(os.path.join(ROOT, "include", "reef_msm.h")).read())
    protos = {}
    for m in re.finditer(r"\b([\w ]+?[\s\*]+)((?:reef_|mult_pippenger_)\w+)\s*\(([^;{}]*?)\)\s*;", hdr):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()

        def kind(a):
            a = a.strip()
            if "*" in a or a.endswith("]"):
                return "ptr"
            return C_KINDS[a.rsplit(" ", 1)[0].replace("const", "").strip()]
        protos[name] = ("ptr" if "*" in ret else C_KINDS[ret], [kind(a) for a in args.split(",")] if args not in ("", "void") else [])
    return protos


def rust_kind(t):
    t = t.strip()
    return "ptr" if t.startswith("*") else t
