"""Float64 numpy restatement of the weight average of nextbestpath_amd/optim.py::WeightEMA (csrc/nbp_ema.hip), and the
rounding-error bound the fp32 kernel is held to.

    d  = min(decay, (1 + n) / (10 + n))   with warm-up, after n applied updates;   d = decay without
    e' = e + (1 - d) (p - e)

`d` is the same IEEE double on the host and on the device: a quotient of two small integers, then a min."""
import numpy as np


def decay_at(decay, n, warmup=True):
    """The decay of the update that follows n applied ones."""
    decay = float(decay)
    if not warmup:
        return decay
    return min(decay, (1.0 + n) / (10.0 + n))


def ema_step(e, p, decay, n, warmup=True):
    """One update of one tensor in float64 from inputs of any float dtype.  -> e'"""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    d = decay_at(decay, n, warmup)
    return e + (1.0 - d) * (p - e)


def bound(e, p, ref):
    """The absolute error allowed on e' for a kernel that evaluates the rule in double from the fp32 operands and rounds once:
        |got - e64'| <= 2^-24 |e64'| + 2^-45 (|e| + |p|)
    The first term is the one fp32 rounding of the result.  The second covers the <= 3 double roundings of the expression (each
    2^-53 of a quantity no larger than |e| + |p|, with a factor of 2^5 to spare) in whichever association it is written --
    e + (1 - d)(p - e), the same with a fused multiply-add, or d e + (1 - d) p -- and the restatement's own."""
    e, p = np.abs(np.asarray(e, dtype=np.float64)), np.abs(np.asarray(p, dtype=np.float64))
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -45 * (e + p)
