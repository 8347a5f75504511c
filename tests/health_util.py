"""Shared by tests/test_health_cpu.py and tests/test_health_gpu.py: numpy's summation order of
np.mean restated in plain Python, and the fixed health inputs both tests use."""
import numpy as np

NP_CHUNK = 8192   # elements per pairwise sum of np.mean's buffered reduction
PW_BLOCK = 128    # numpy's PW_BLOCKSIZE

SIZES = [1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 569, 2276, 8192, 8193, 9102]
# seeds at which plain pairwise summation over the whole list differs from np.mean (the chunked
# rule) at the two sizes past one chunk: found by trying seeds 0, 1, 2, ... in order
SEEDS = {8193: 0, 9102: 1}


def healths(n, seed=None):
    """rng.random(n) * 100 under the size's fixed seed."""
    seed = SEEDS.get(n, 1000 + n) if seed is None else seed
    return np.random.default_rng(seed).random(n) * 100


def pairwise(a):
    """numpy's DOUBLE_pairwise_sum over a list of Python floats (IEEE f64 adds)."""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res = res + v
        return res
    if n <= PW_BLOCK:
        r = list(a[:8])
        body = n - n % 8
        for i in range(8, body, 8):
            for k in range(8):
                r[k] = r[k] + a[i + k]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(body, n):
            res = res + a[i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:n2]) + pairwise(a[n2:])


def chunked_mean(a):
    """np.mean of a 1-D f64 list: consecutive chunks of NP_CHUNK, each summed pairwise, the chunk
    sums added left to right onto the first, the total divided by n. nan for an empty list."""
    a = [float(v) for v in a]
    if not a:
        return float("nan")
    total = pairwise(a[:NP_CHUNK])
    for c0 in range(NP_CHUNK, len(a), NP_CHUNK):
        total = total + pairwise(a[c0:c0 + NP_CHUNK])
    return total / len(a)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)
