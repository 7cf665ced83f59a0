"""What the Python front-ends share: the lifetime of an opaque handle of the C ABI, and field elements as they cross it --
Python ints <-> (n, 4) uint64 arrays of little-endian limbs, canonical <-> pasta Montgomery form."""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import numpy as np


class _Handle:
    """close / with / garbage collection for a class that sets `_lib` and `_h` and names the ABI's destroy entry in `_destroy`."""
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _arr(vals: Sequence[int]) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def _ints(a: np.ndarray) -> List[int]:
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _mont_forms(p: int, is_mont: bool) -> Tuple[Callable[[int], int], Callable[[int], int]]:
    """(to, frm): a canonical int to the form the library is called with (pasta Montgomery form when is_mont), and back."""
    if not is_mont:
        return (lambda v: v), (lambda v: v)
    R = (1 << 256) % p
    Rinv = pow(R, -1, p)
    return (lambda v: v * R % p), (lambda v: v * Rinv % p)
