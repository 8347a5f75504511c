"""Every case of the GEMM / conv3x3 route tables (gemm_route_cases.py) plans as it says, on a host
without a GPU: evx_gemm_plan_query is the function gemm_launch itself switches on, asked with fake
non-null pointers (0x1000: 16-byte aligned, 0x1004: not). The GPU test launches the same
descriptors; this file is what holds the tables' routes, slice counts and reductions, and that
every EVX_ROUTE_* of the header has a case."""
import ctypes
import os
import re

import pytest
import torch

from gemm_route_cases import CONV_CASES, GEMM_CASES, check_plan, conv_args, conv_dims, gemm_args, gemm_ws
from golden_util import ROOT

ALIGNED, UNALIGNED = 0x1000, 0x1004


class Fake:
    """Stands for a device tensor: an address, and the host as its device (the workspace pool's)."""
    device = torch.device("cpu")

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def gemm_case_desc(c):
    from evacx import qnet
    A = Fake(ALIGNED + 4 * c.opts.get("a_off", 0))
    assert A.addr in (ALIGNED, UNALIGNED)
    return qnet.gemm_desc(**gemm_args(c, A, Fake(ALIGNED), Fake(0x3000), bias=Fake(0x4000) if "b" in c.epi else None,
                                      mask=Fake(0x5000) if "m" in c.epi else None,
                                      gate=Fake(0x6000) if "g" in c.epi else None, ws=gemm_ws(c, "cpu")))


def conv_case_desc(c):
    from evacx import qnet
    ws = qnet._Workspace() if c.opts.get("ws") else None
    return qnet.conv_desc(**conv_args(c, Fake(ALIGNED), Fake(ALIGNED), Fake(0x3000),
                                      bias=Fake(0x4000) if c.mode == "fwd" else None,
                                      gate=Fake(0x6000) if c.opts.get("gate") else None, ws=ws))


@pytest.mark.parametrize("c", GEMM_CASES, ids=lambda c: c.name)
def test_gemm_case_plans_as_intended(c):
    from evacx import qnet
    check_plan(c, qnet.gemm_plan(gemm_case_desc(c)))


@pytest.mark.parametrize("c", CONV_CASES, ids=lambda c: c.name)
def test_conv_case_plans_as_intended(c):
    from evacx import qnet
    mode, _, _, _, cs = conv_dims(c)
    check_plan(c, qnet.gemm_plan(conv_case_desc(c), mode, cs))


def test_case_names_are_unique():
    names = [c.name for c in GEMM_CASES + CONV_CASES]
    assert len(set(names)) == len(names)


def test_every_route_and_reduction_has_a_case():
    """A route added to the header later fails here until the tables give it a case. EVX_ROUTE_NONE
    (nothing to launch) is the empty GEMM below."""
    from evacx import _lib, qnet
    text = open(os.path.join(ROOT, "include", "evacx.h")).read()
    routes = set(re.findall(r"#define EVX_ROUTE_(\w+)", text))
    reduces = set(re.findall(r"#define EVX_REDUCE_(\w+)", text))
    assert routes == set(_lib.ROUTE) and reduces == set(_lib.REDUCE)
    d = qnet.gemm_desc(0, 4, 4, Fake(ALIGNED), 4, 1, Fake(ALIGNED), 1, 4, Fake(0x3000), 4, "x3")
    p = qnet.gemm_plan(d)
    assert (p.route, p.slices, p.klen, p.reduce) == (_lib.ROUTE["NONE"], 0, 0, _lib.REDUCE["NONE"])
    cases = GEMM_CASES + CONV_CASES
    assert {c.route for c in cases} | {"NONE"} == routes
    assert {c.reduce for c in cases} == reduces


def _query(d, mode=0, cs=0):
    from evacx import _lib
    L = _lib.lib()
    p = _lib.evx_gemm_plan()
    rc = L.evx_gemm_plan_query(ctypes.byref(d), mode, cs, ctypes.byref(p))
    return rc, L.evx_q_last_error(), p


def _fwd_desc(Mp, cin, cout, **kw):
    from evacx import qnet
    return qnet.conv_desc(qnet.CONV_FWD, Mp, cout, 9 * cin, Fake(ALIGNED), Fake(ALIGNED), Fake(0x3000), cin, sbk=9,
                          sbn=9 * cin, bias=Fake(0x4000), relu=True, **kw)


def test_argument_errors_come_back_as_the_launch_reports_them():
    from evacx import _lib, qnet
    A, B, Cm = Fake(ALIGNED), Fake(ALIGNED), Fake(0x3000)
    # OUT_SPLIT without a staged route: no workspace, and a shape the staged kernels do not take
    for d, cs in ((_fwd_desc(121, 64, 128, out_split=True), 64),
                  (_fwd_desc(121, 5, 7, out_split=True, ws=qnet._Workspace()), 5)):
        rc, text, p = _query(d, qnet.CONV_FWD, cs)
        assert rc == -22 and b"OUT_SPLIT needs the LDS-staged conv forward" in text, text
        assert p.route == _lib.ROUTE["NONE"]
    d = qnet.gemm_desc(8, 8, 16, A, 16, 1, B, 1, 16, Cm, 8, "x3")
    d.flags |= _lib.OUT_SPLIT
    rc, text, _ = _query(d)
    assert rc == -22 and b"OUT_SPLIT" in text
    # SPLIT_AB: K % 8 != 0, and precisions other than x3
    rc, text, _ = _query(qnet.gemm_desc(8, 8, 12, A, 16, 1, B, 1, 16, Cm, 8, "x3", split_ab=True))
    assert rc == -22 and b"SPLIT_AB needs x3, k-contiguous operands, K and row strides multiples of 8" in text
    rc, text, _ = _query(qnet.gemm_desc(8, 8, 16, A, 16, 1, B, 1, 16, Cm, 8, "bf16", split_ab=True))
    assert rc == -22 and b"SPLIT_AB needs x3" in text
    assert _query(qnet.gemm_desc(8, 8, 16, A, 16, 1, B, 1, 16, Cm, 8, "x3", split_ab=True))[0] == 0
    # conv: pixel rows not 121 * B, taps x channels, mode, precision
    rc, text, _ = _query(_fwd_desc(120, 6, 32), qnet.CONV_FWD, 6)
    assert rc == -22 and b"conv3x3: pixel count not 121*B" in text
    rc, text, _ = _query(_fwd_desc(121, 6, 32), qnet.CONV_FWD, 5)
    assert rc == -22 and b"taps x channels mismatch" in text
    rc, text, _ = _query(_fwd_desc(121, 6, 32), 4, 6)
    assert rc == -22 and b"conv3x3: bad mode" in text
    d = _fwd_desc(121, 6, 32)
    d.precision = _lib.PREC["f32"]
    rc, text, _ = _query(d, qnet.CONV_FWD, 6)
    assert rc == -22 and b"x3 only" in text
    # evx_gemm's own: a NULL operand, a negative workspace size; the query's NULL plan
    d = qnet.gemm_desc(8, 8, 16, A, 16, 1, B, 1, 16, Cm, 8, "x3")
    d.B = None
    rc, text, _ = _query(d)
    assert rc == -22 and b"gemm: NULL operand" in text
    d = qnet.gemm_desc(8, 8, 16, A, 16, 1, B, 1, 16, Cm, 8, "x3")
    d.ws_elems = -1
    rc, text, _ = _query(d)
    assert rc == -22 and b"ws_elems < 0" in text
    assert _lib.lib().evx_gemm_plan_query(ctypes.byref(d), 0, 0, None) == -22


def test_the_launch_reports_the_same_error_without_touching_a_device():
    """evx_gemm / evx_conv3x3_gemm fail in the plan, before any launch: the same code and text."""
    from evacx import _lib, qnet
    L = _lib.lib()
    d = qnet.gemm_desc(8, 8, 12, Fake(ALIGNED), 16, 1, Fake(ALIGNED), 1, 16, Fake(0x3000), 8, "x3", split_ab=True)
    rc, text, _ = _query(d)
    assert L.evx_gemm(ctypes.byref(d), None) == rc == -22 and L.evx_q_last_error() == text
    d = _fwd_desc(120, 6, 32)
    rc, text, _ = _query(d, qnet.CONV_FWD, 6)
    assert L.evx_conv3x3_gemm(ctypes.byref(d), qnet.CONV_FWD, 6, None) == rc == -22 and L.evx_q_last_error() == text
    d = _fwd_desc(121, 64, 128, out_split=True)
    rc, text, _ = _query(d, qnet.CONV_FWD, 64)
    assert L.evx_conv3x3_gemm(ctypes.byref(d), qnet.CONV_FWD, 64, None) == rc == -22 and L.evx_q_last_error() == text
