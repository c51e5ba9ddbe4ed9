"""The value of a learning-rate schedule (include/dfwfm_lr_schedule.h) in exact rational arithmetic.

Every intermediate is a fractions.Fraction and is rounded to a float exactly where the contract rounds -- the two
int64 -> double conversions, their quotient, the rates' difference, and the fused multiply-add as ONE rounding of the
exact product plus the exact addend -- and nowhere else.  Python's Fraction -> float conversion is correctly rounded
(round to nearest, ties to even), so this is a true fma without math.fma."""
from fractions import Fraction


def _rn(x):
    """The double nearest to the exact rational x."""
    return float(Fraction(x))


def lr_at(knots, s):
    """The schedule [(step, lr), ...] at step s: lr[0] up to the first knot, lr[n-1] from the last one, else on
    step[i] <= s < step[i+1]: t = rn(rn(s - step[i]) / rn(step[i+1] - step[i])), lr = rn((lr[i+1] - lr[i])_rn * t + lr[i])."""
    steps = [int(k[0]) for k in knots]
    lrs = [float(k[1]) for k in knots]
    s = int(s)
    if s <= steps[0]:
        return lrs[0]
    if s >= steps[-1]:
        return lrs[-1]
    i = max(j for j in range(len(steps) - 1) if steps[j] <= s)
    num = _rn(s - steps[i])                               # (double)(s - step[i]): the integer difference is exact
    den = _rn(steps[i + 1] - steps[i])
    t = _rn(Fraction(num) / Fraction(den))
    d = _rn(Fraction(lrs[i + 1]) - Fraction(lrs[i]))
    return _rn(Fraction(d) * Fraction(t) + Fraction(lrs[i]))  # one rounding: the fma


def bits(x):
    """The 64 bits of a double (so that +0.0 / -0.0 and NaN payloads compare as bits)."""
    import struct
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]
