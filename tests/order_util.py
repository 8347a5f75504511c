"""The scheduling permutations restated in numpy on the state words (scal [E][4]: fire step at
[e][0], persons evacuated / dead at [e][2] / [e][3]), shared by test_order_gpu.py and the fused
launch's tests in test_replay_gpu.py."""
import numpy as np


def random_scal(E, P, t_max, rng):
    """State words with fire steps on both sides of t_max and every number of persons remaining."""
    scal = np.zeros((E, 4), np.int32)
    scal[:, 0] = rng.integers(0, t_max + 3, E)
    ev = rng.integers(0, P + 1, E)
    scal[:, 2] = ev
    scal[:, 3] = np.minimum(rng.integers(0, P + 1, E), P - ev)
    return scal


def want_classes(scal, P, t_max):
    """One class byte per env: bucket of persons remaining | 0x10 fire class | 0x20 heavy."""
    rem = P - scal[:, 2] - scal[:, 3]
    b = 15 - np.minimum(15, np.maximum(0, rem) * 16 // (P + 1))
    return (b | np.where(scal[:, 0] >= t_max, 0x10, 0) | np.where(rem >= max(1, P // 4), 0x20, 0)).astype(np.uint8)


def want_perm(scal, t_max):
    """evx_act_perm: the stable partition of the envs by fire step >= t_max."""
    sel = scal[:, 0] >= t_max
    return np.concatenate([np.nonzero(sel)[0], np.nonzero(~sel)[0]]).astype(np.int32)


def want_order(scal, P):
    """evx_env_order: (the stable counting sort by 16 buckets of persons remaining, heaviest first;
    order[E], the heavy count min(176, #envs with >= P/4 persons remaining))."""
    rem = P - scal[:, 2] - scal[:, 3]
    bucket = 15 - np.minimum(15, np.maximum(0, rem) * 16 // (P + 1))
    return np.argsort(bucket, kind="stable").astype(np.int32), min(176, int(np.sum(rem >= max(1, P // 4))))
