"""The step kernel's dynamic LDS per env from the host function the launch uses
(evx_step_lds_bytes; no GPU): the benchmark layout stays within 10 LDS allocation granules of
1280 B, so that 12 one-wave workgroups fit the 128 granules of a CU."""
import ctypes as C

GRANULE = 1280


def _lds_bytes(grid, P, R):
    from evacx import _lib
    lay = _lib.evx_layout(L=grid, W=grid, P=P, R=R)
    for k in ["floor", "cellinfo", "valid_bits", "danger_p", "danger_o"]:
        setattr(lay, k, 8)  # any non-NULL value: the size query reads no table
    return _lib.lib().evx_step_lds_bytes(C.byref(lay))


def test_bench_layout_fits_twelve_envs_per_cu():
    b = _lds_bytes(128, 2276, 16)  # cfg3
    assert b == 12800
    assert 12 * -(-b // GRANULE) <= 128


def test_other_layouts_lds_bytes():
    # 2 x 624 MT rings + 528 aux + 3 grid bitmaps at 1, 1 and 1/4 bit per cell + losers + robots + 144 misc
    assert _lds_bytes(64, 569, 8) == 9024     # cfg2
    assert _lds_bytes(128, 2276, 32) == 12864  # cfg5: 11 granules (its 8192-env bench runs 4-wave workgroups)
    assert _lds_bytes(178, 1500, 2) == 21056  # the largest grid with its bitmaps in LDS
