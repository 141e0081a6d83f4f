"""The exact raster sum's definition (include/uampath.h, "Exact, order-independent raster
sums") in Python integers and fractions.Fraction: the independent reference of
test_exact_sum_cpu.py and test_gpu_exact_sum.py.  It shares no code with the library.

Values are float32 bit patterns (ints): words(a) takes them from anything numpy reads as
float32."""
from fractions import Fraction

import numpy as np

NAN, PINF, NINF = 1, 2, 4   # a field's side flags


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32).tolist()


def _b(w):
    return (w >> 23) & 255


def exponent(ws):
    """e = max(1, largest biased exponent field among the finite words) - 126."""
    return max([1] + [_b(w) for w in ws if _b(w) != 255]) - 126


def flags(ws):
    f = 0
    for w in ws:
        if _b(w) == 255:
            f |= NAN if w & 0x7FFFFF else NINF if w >> 31 else PINF
    return f


def term(w, e):
    """A finite word's term in quanta of 2^(e - 96); a right shift truncates the magnitude."""
    b = _b(w)
    assert b != 255
    M = (w & 0x7FFFFF) | (0x800000 if b else 0)
    sh = max(b, 1) - 54 - e
    assert sh <= 72, "the exponent does not cover this value"
    t = M << sh if sh >= 0 else M >> -sh
    assert t < 1 << 96
    return -t if w >> 31 else t


def truncated(w, e):
    """Whether term(w, e) lost bits of w."""
    b = _b(w)
    M = (w & 0x7FFFFF) | (0x800000 if b else 0)
    sh = max(b, 1) - 54 - e
    return sh < 0 and (M >> -sh) << -sh != M


def fl(S, e):
    """S 2^(e - 96) rounded once to float64, to nearest even (CPython's int / int is correctly
    rounded); S = 0 gives +0.0."""
    assert -(1 << 127) <= S < 1 << 127
    x = Fraction(S) * Fraction(2) ** (e - 96)
    return x.numerator / x.denominator


def result(S, f, e):
    if f & NAN or (f & PINF and f & NINF):
        return float("nan")
    if f & PINF:
        return float("inf")
    if f & NINF:
        return float("-inf")
    return fl(S, e)


def exact_sum(ws, e=None):
    """(result, e, flags) of the words ws; e=None derives the exponent from them."""
    if e is None:
        e = exponent(ws)
    S = sum(term(w, e) for w in ws if _b(w) != 255)
    f = flags(ws)
    return result(S, f, e), e, f
