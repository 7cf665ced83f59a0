"""Reference model of reef_doc_transform (include/reef_msm.h 3l), written from its definition; Python's own strict decoder is the UTF-8
authority (it follows the rule Rust's from_utf8 follows).  Shared by tests/test_doc_host.py and tests/test_gpu_doc_transform.py."""
import numpy as np

BYTES, UTF8 = 0, 1
DROP, BAD = 0xFFFFFFFE, 0xFFFFFFFF


def next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


def own_symbols(c: np.ndarray, encoding: int, eof: int) -> np.ndarray:
    """map == NULL: the encoding's own alphabet"""
    v = np.where(c < 128, c, BAD) if encoding == BYTES else np.where(c < 0xD800, c, c - 0x800)
    return np.where(c == 0x1A, eof, v).astype(np.uint32)


def characters(text: bytes, encoding: int):
    """-> (character values, their byte offsets, malformed_at) as numpy arrays; for malformed UTF-8 the characters of the well-formed prefix"""
    if encoding == BYTES:
        return np.frombuffer(text, dtype=np.uint8).astype(np.uint32), np.arange(len(text), dtype=np.int64), len(text)
    try:
        s, malformed_at = text.decode("utf-8"), len(text)
    except UnicodeDecodeError as e:
        s, malformed_at = text[:e.start].decode("utf-8"), e.start
    c = np.frombuffer(s.encode("utf-32-le"), dtype=np.uint32)
    width = 1 + (c >= 0x80) + (c >= 0x800) + (c >= 0x10000)
    return c, np.cumsum(width) - width, malformed_at


def transform(text: bytes, encoding: int, map_, eof: int, epsilon: int):
    """transform_array with the symbols as a list"""
    syms, info = transform_array(text, encoding, map_, eof, epsilon)
    return (None if syms is None else [int(x) for x in syms]), info


def transform_array(text: bytes, encoding: int, map_, eof: int, epsilon: int):
    """-> (symbols as a uint32 array, or None when nothing is written; info as a dict).  bad / first_bad are defined for well-formed text only."""
    c, at, malformed_at = characters(text, encoding)
    n = len(text)
    if malformed_at < n:
        return None, {"malformed_at": malformed_at}
    if map_ is None:
        v = own_symbols(c, encoding, eof)
    else:
        m = np.asarray(map_, dtype=np.uint32)
        v = np.where(c < len(m), m[np.minimum(c, len(m) - 1)], BAD).astype(np.uint32)
    is_bad = v == BAD
    bad = int(is_bad.sum())
    kept = int((v != DROP).sum())    # "characters not dropped": a BAD character is not dropped
    info = {"chars": len(c), "kept": kept, "padded": next_pow2(kept + 2), "bad": bad, "first_bad": int(at[is_bad][0]) if bad else n, "malformed_at": n}
    if bad:
        return None, info
    out = np.zeros(info["padded"], dtype=np.uint32)
    out[:kept] = v[v != DROP]
    out[kept], out[kept + 1] = eof, epsilon
    return out, info


def doc_transform(ab: str, doc: str):
    """framework.rs:978 restated from the issue's definition: position in the alphabet (a later duplicate wins), 0x1A -> len + 2"""
    table = {}
    for i, c in enumerate(ab):
        table[c] = i
    table["\x1a"] = len(ab) + 2
    out = [table[c] for c in doc] + [len(ab) + 2, len(ab) + 1]
    return out + [0] * (next_pow2(len(out)) - len(out))


def as_array(symbols, elem_bytes: int) -> np.ndarray:
    return np.array(symbols, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[elem_bytes])
