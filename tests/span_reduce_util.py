"""The span reduce's stated order (include/evacx.h at evx_episode_reduce, csrc/evx_reduce.h),
restated once in numpy for every test that holds a reduce to it bit for bit.

Thread t of SPAN takes the member envs t, t + SPAN, ... in ascending order onto its start value
(0.0 for a sum, +inf / -inf for min / max; the others are skipped), then s[t] = op(s[t], s[t + h])
for h = SPAN/2 .. 1 and the result is s[0]. min and max keep the kernel's comparisons (b < a ? b : a
and b > a ? b : a). A row without members gives the start value."""
import numpy as np

SPAN = 1024  # EVX_EPISODE_REDUCE_SPAN


def _span(vals, member, start, op):
    vals = np.asarray(vals, np.float64)
    s = np.full(SPAN, start, np.float64)
    with np.errstate(all="ignore"):
        for e in np.nonzero(np.asarray(member, bool))[0]:  # ascending, so ascending per thread
            s[e % SPAN] = op(s[e % SPAN], vals[e])
        h = SPAN // 2
        while h:
            s[:h] = op(s[:h], s[h:2 * h])
            h //= 2
    return s[0]


def span_sum(vals, member):
    return _span(vals, member, 0.0, lambda a, b: a + b)


def span_min(vals, member):
    return _span(vals, member, np.inf, lambda a, b: np.where(b < a, b, a))


def span_max(vals, member):
    return _span(vals, member, -np.inf, lambda a, b: np.where(b > a, b, a))
