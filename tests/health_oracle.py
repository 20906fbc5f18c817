"""The numpy restatement of the numerical-health records (include/vtd.h "Numerical health") and
of the reference diagnostics built on them, with the designed vectors the tests use.

A record of a float32 array x:
  n, nan, pos_inf, neg_inf   the element count and how many elements are NaN / +inf / -inf
  max, min                   over the elements that are not NaN, infinities included; with no such
                             element max = -inf and min = +inf.  Compared by VALUE by the tests,
                             so +0 and -0 are equal.  Subnormals are kept.
  sumsq                      the sum of (double)x * (double)x over the finite elements.  A float32
                             has a 24-bit significand, so the fp64 square is exact; here the exact
                             squares are added with math.fsum, which returns the correctly rounded
                             exact sum.
The bound for a device sumsq: every term is >= 0 and exactly representable, so any summation
order in fp64 commits at most n - 1 roundings, each at most 2^-53 relative to a partial sum that
never exceeds the total: within (n - 1) 2^-53 of the exact sum, and math.fsum is within 2^-53 of
it -- together n * 2^-53 relative (`sumsq_bound`).  Derived, not measured.
"""
import math
from collections import OrderedDict

import numpy as np

NS = lambda c: (1, 3, 4, 5, 255, 256, 257, 1023, 1025, c - 1, c, c + 1, 2 * c + 7)   # noqa: E731
OFFSETS = (0, 1, 2, 3)                   # floats past a 16-B boundary: 0 / 4 / 8 / 12 bytes
PATTERNS = ("plain", "special_0", "special_1", "special_2", "all_nan", "subnormal_max",
            "negzero_max")


def stats64(x):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    nan = np.isnan(x)
    kept = x[~nan]
    finite = x[np.isfinite(x)].astype(np.float64)
    return dict(n=int(x.size), nan=int(nan.sum()), pos_inf=int((x == np.inf).sum()),
                neg_inf=int((x == -np.inf).sum()),
                max=np.float32(kept.max()) if kept.size else np.float32(-np.inf),
                min=np.float32(kept.min()) if kept.size else np.float32(np.inf),
                sumsq=math.fsum(finite * finite))


def sumsq_bound(want):
    """The allowed absolute deviation of a device sumsq from stats64's (module docstring)."""
    return want["n"] * 2.0 ** -53 * want["sumsq"]


def norm(want):
    if want["nan"]:
        return float("nan")
    if want["pos_inf"] or want["neg_inf"]:
        return float("inf")
    return math.sqrt(want["sumsq"])


def mismatch(got, want):
    """'' if the record `got` (an object with the record's fields) equals the oracle's `want`:
    the exact fields exactly (max / min by value), sumsq within the bound; else what differs."""
    bad = [f for f in ("n", "nan", "pos_inf", "neg_inf") if getattr(got, f) != want[f]]
    bad += [f for f in ("max", "min") if not float(getattr(got, f)) == float(want[f])]
    if not abs(got.sumsq - want["sumsq"]) <= sumsq_bound(want):
        bad.append("sumsq")
    return ", ".join(f"{f}: {getattr(got, f)!r} != {want[f]!r}" for f in bad)


def replace(x, r):
    """x with every NaN replaced by float32(r); every other element keeps its bits."""
    x = np.ascontiguousarray(x, np.float32)
    out = x.copy()
    out[np.isnan(x)] = np.float32(r)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the reference's arithmetic
def check_weights_ref(weights):
    """vtd.py:744-748 on a dict of arrays: starts from 0, `max_weight < np.amax(weight)`; np.amax
    of an array holding a NaN is NaN and the comparison is then False."""
    max_weight = 0
    for w in weights.values():
        if max_weight < np.amax(w):
            max_weight = np.amax(w)
    return max_weight


class CheckModelWeightRef:
    """vtd.py:654-687's bookkeeping on dicts of arrays, with the maximum / minimum over the
    non-NaN elements (the record's; -inf / +inf when there is none)."""

    def __init__(self, start_epochs, skip_epochs, weight_threshold):
        self.max_weight, self.min_weight = weight_threshold, -weight_threshold
        self.start_epochs, self.skip_epochs = start_epochs, skip_epochs
        self.checked = []

    def due(self, epoch):
        return (epoch >= self.start_epochs) and ((epoch - self.start_epochs) % self.skip_epochs
                                                 == 0)

    def on_epoch_end(self, epoch, weights):
        if not self.due(epoch):
            return
        self.checked.append(epoch)
        for w in weights.values():
            w = np.asarray(w, np.float32).reshape(-1)
            kept = w[~np.isnan(w)]
            mx = float(kept.max()) if kept.size else -math.inf
            mn = float(kept.min()) if kept.size else math.inf
            if mx > self.max_weight:
                self.max_weight = mx
            elif mn < self.min_weight:
                self.min_weight = mn


# ------------------------------------------------------------------ designed vectors
def magnitudes(rng, n):
    """Signed values with magnitudes from 1e-20 to 1e19 in one tensor: in fp32 their squares
    underflow (1e-40) and a few of the largest (1e38) already sum past the format's maximum; in
    fp64 neither happens."""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-20.0, 19.0, n)).astype(np.float32)


def design(pattern, n, c, seed):
    """One designed vector of n elements for chunk size c."""
    rng = np.random.default_rng([seed, n, PATTERNS.index(pattern)])
    x = magnitudes(rng, n)
    if pattern == "plain":
        return x
    if pattern.startswith("special_"):
        # NaN, +inf and -inf at element 0, at the last element and on both sides of every chunk
        # boundary the vector has; the three patterns rotate which special sits where
        r = int(pattern[-1])
        specials = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))
        spots = [0, n - 1] + [p for k in (1, 2) for p in (k * c - 1, k * c)]
        for k, p in enumerate(spots):
            if 0 <= p < n:
                x[p] = specials[(k + r) % 3]
        return x
    if pattern == "all_nan":
        x[:] = np.nan
        return x
    x = -np.abs(x)                                   # every element negative (none is zero)
    assert (x < 0).all()
    spot = int(rng.integers(n))
    if pattern == "subnormal_max":
        x[spot] = np.float32(3e-42)                  # a subnormal: flushed, the max would be 0
        assert 0 < x[spot] < np.finfo(np.float32).tiny
    else:                                            # negzero_max
        x[spot] = np.float32(-0.0)
    return x


def designs(c, seed=7):
    """OrderedDict name -> (offset in floats past a 16-B boundary, vector): every n of NS(c) x
    every offset x every pattern."""
    out = OrderedDict()
    for n in NS(c):
        for off in OFFSETS:
            for p in PATTERNS:
                out[f"{p}/n{n}/o{off}"] = (off, design(p, n, c, seed + off))
    return out


def layout(table, guard=8):
    """Places the designed vectors in one float32 buffer, each at its offset past a 16-B boundary
    and `guard` sentinel floats apart.  Returns (buffer, {name: (start, n)}); the sentinel is
    a value no design holds."""
    spans, pos = OrderedDict(), guard
    for name, (off, x) in table.items():
        pos = (pos + 3) // 4 * 4 + off
        spans[name] = (pos, x.size)
        pos += x.size + guard
    buf = np.full(pos + guard, SENTINEL, np.float32)
    for name, (off, x) in table.items():
        s, n = spans[name]
        buf[s:s + n] = x
    return buf, spans


SENTINEL = np.float32(-12345.678)
