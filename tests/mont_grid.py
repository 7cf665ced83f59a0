"""The operand grid of the Montgomery-reduction tests: nine 29-bit limbs at the limb and value bounds field.h states, the exact
integer the reduction defines, and the check of a result's limbs.  Shared by tests/test_mont_reduction.py (the host build of the
templates) and tests/test_gpu_field_bounds.py (the same grid on the device)."""
MASK = (1 << 29) - 1
RP = 1 << 261


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def mont(t, m):
    q = (-t * pow(m, -1, RP)) % RP
    assert (t + q * m) % RP == 0
    return (t + q * m) // RP


def operand(rng, m, bound, kind):
    """Nine limbs, normalised (limb 0 < 2^29, limbs 1..7 <= 2^29 + 7), value < bound * M."""
    lim = int(bound * m) - 1
    if kind == "zero":
        return [0] * 9
    if kind == "max":      # every low limb at its bound, the top limb as large as the value bound allows
        low = [MASK] + [MASK + 8] * 7
    elif kind == "top":    # canonical low limbs, value just below the bound
        v = lim - int(rng.integers(0, 1 << 20))
        return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]
    else:
        low = [int(rng.integers(0, 1 << 29))] + [int(rng.integers(0, MASK + 9)) for _ in range(7)]
    rest = lim - value(low + [0])
    assert rest >= 0
    top_max = rest >> 232
    top = top_max if kind == "max" else int(rng.integers(0, top_max + 1))
    return low + [top]


KINDS = ["max", "top", "zero"] + ["rand"] * 61


def check_limbs(r, m, vmax, want):
    assert all(int(x) <= MASK for x in r[:8]), [hex(int(x)) for x in r]
    v = value(r)
    assert v == want, (hex(v), hex(want))
    assert v < vmax * m


# (A/M, B/M) pairs with (A/M)(B/M) < 128: balanced, lopsided, and the operands of the group law (ec.h: 9.02 x 5.04)
PAIRS = [(1.0, 1.0), (2.0, 2.0), (11.3, 11.3), (2.0, 63.9), (1.0, 127.9), (9.02, 5.04), (5.2, 5.2)]
