#!/usr/bin/env python3
"""Diagnostic, launches no kernel: the LDS step sizes of the device as the runtime's occupancy
query sees them (evx_env_step_occupancy). The step kernel's dynamic LDS is swept through throw-away
layouts -- a 128x128 / 120x120 / 112x112 grid with P from 32 to 16383 changes the `lost` bitmap by
one word per 32 persons -- and every change of workgroups per CU is printed with the LDS bytes on
both sides of it. The residency plateau of tools/stamp_probe.py is the arbiter where the query
does not model the allocation granule."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqn-marl_amd"))

from evacx import _lib  # noqa: E402
from evacx.env import DeviceLayout  # noqa: E402
from evacx.layout import build_tables, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grids", type=int, nargs="+", default=[128, 120, 112])
ap.add_argument("--robots", type=int, default=16)
ap.add_argument("--envs", type=int, default=32768, help="E of the launch (>= 64 per CU: one-wave workgroups)")
args = ap.parse_args()

L = _lib.lib()


def query(layc, P):
    c = _lib.evx_layout.from_buffer_copy(layc)
    c.P = P
    st = _lib.evx_state(E=args.envs)
    n, lds, thr = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(L.evx_env_step_occupancy(C.byref(c), C.byref(st), C.byref(n), C.byref(lds), C.byref(thr)),
               "evx_env_step_occupancy")
    return n.value, lds.value, thr.value


for grid in args.grids:
    lay = DeviceLayout(build_tables(synthetic(grid, grid, args.robots)), 2276)
    prev = None
    print(f"grid {grid}x{grid}, R {args.robots}, E {args.envs}:")
    for P in range(32, 16384, 32):
        n, lds, thr = query(lay.c, P)
        if prev is None:
            print(f"  P {P:5d}: {lds:6d} B, {thr} threads -> {n} workgroups per CU")
        elif n != prev[0]:
            print(f"  {prev[1]:6d} B -> {prev[0]:2d} per CU | {lds:6d} B -> {n:2d} per CU   (P {P})")
        prev = (n, lds)
    print(f"  P 16383: {prev[1]:6d} B -> {prev[0]} per CU")
    n, lds, thr = query(lay.c, 2276)
    print(f"  P 2276 (the bench's): {lds} B, {thr} threads -> {n} workgroups per CU")
