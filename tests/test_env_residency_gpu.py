"""The step kernel's LDS layout after the contested-target prefilter went to quarter resolution
(12 one-wave workgroups per CU at 128x128 instead of 11): bit-exact against the C oracle at the
shapes where an LDS region changes role or size, and the occupancy query.

* 178x178: the largest grid with its bitmaps in LDS (1013 words > the 624-word MT ring, so the
  vacated-cell bitmap no longer overlays the Python ring);
* 160x160 crowded (contested targets), single-wave and wide rows;
* 30x14: G = 512 cells, no slack bits at the end of any bitmap, fused auto-reset;
* 24x20 dense: the conflict-heavy shape, every step checked, also on one-wave workgroups (the
  variant a 32768-env launch uses);
* evx_env_step_occupancy at the benchmark layout.
"""
import ctypes as C

import pytest
import torch

from test_env_gpu import _need_gpu, _oracle_pair

pytestmark = pytest.mark.gpu


def test_largest_lds_grid_178_vs_oracle():
    _need_gpu()
    from evacx.layout import synthetic
    _oracle_pair(synthetic(178, 178, 2), 1500, E=2, steps=20)


@pytest.mark.parametrize("wide", [False, True])
def test_crowded_160_vs_oracle(wide):
    _need_gpu()
    from evacx.layout import synthetic
    _oracle_pair(synthetic(160, 160, 4), 3000, E=3, steps=25, wide=wide)
    if wide:
        assert _oracle_pair.max_heavy == 3  # the 4-wave workgroup still fits in LDS


def test_no_slack_bitmaps_30x14_auto_reset_vs_oracle():
    _need_gpu()
    from evacx.layout import synthetic
    spec = synthetic(30, 14, 2)
    assert (spec.L + 2) * (spec.W + 2) == 512
    n = _oracle_pair(spec, 120, E=8, steps=60, act_seed=1, auto_reset=True)
    assert n == 4  # episode ends the oracle sees with these seeds


@pytest.mark.parametrize("nwb", [None, 1])
def test_dense_conflicts_every_step_vs_oracle(nwb, monkeypatch):
    """nwb = 1: one-wave workgroups (EVX_ENV_NWB), the variant of a launch of >= 64 envs per CU."""
    _need_gpu()
    from evacx import _lib
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    spec = synthetic(24, 20, 4)
    if nwb is not None:
        monkeypatch.setenv("EVX_ENV_NWB", str(nwb))
        lay = DeviceLayout(build_tables(spec), 380)
        assert _occupancy(lay.c, _lib.evx_state(E=16))[2] == 64 * nwb
    _oracle_pair(spec, 380, E=16, steps=50, check_every=1)


def _occupancy(layc, st):
    from evacx import _lib
    n, lds, thr = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().evx_env_step_occupancy(C.byref(layc), C.byref(st), C.byref(n), C.byref(lds), C.byref(thr)),
               "evx_env_step_occupancy")
    return n.value, lds.value, thr.value


def test_occupancy_query_at_bench_layout():
    """32768 envs of cfg3: one-wave workgroups with the LDS of evx_step_lds_bytes, 12 per CU (3 waves
    per SIMD by registers; 12 800 B is 10 LDS allocation granules of 1280 B, 12 x 10 <= 128). Nothing
    is launched: the state holds no buffers."""
    _need_gpu()
    from evacx import _lib
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    lay = DeviceLayout(build_tables(synthetic(128, 128, 16)), 2276)
    torch.cuda.synchronize()
    n, lds, thr = _occupancy(lay.c, _lib.evx_state(E=32768))
    assert thr == 64
    assert lds == _lib.lib().evx_step_lds_bytes(C.byref(lay.c))
    assert lds <= 12800
    assert n >= 12
