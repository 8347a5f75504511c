"""The TD options (Double-Q targets, Huber loss, soft target updates) without a device: the
new C entries exist and validate their arguments before any launch, the Python validator
raises, and the runner's flags and config keys resolve."""
import ctypes as C
import math

import pytest

NEW_SYMBOLS = ["evx_td_loss_opt", "evx_qmlp_td_backward_opt", "evx_polyak", "evx_qmlp_polyak_pack3"]


def test_library_exports_the_new_entries():
    from evacx import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s


def _td_loss_opt(L, opt, Q=None):
    # every pointer NULL (or a non-NULL dummy that is never dereferenced: validation fails first)
    return L.evx_td_loss_opt(Q, None, 5, None, None, None, 0.99, 8, 1, None, None, None, None, None, 0, None, 0,
                             None if opt is None else C.byref(opt), None)


def test_new_entries_validate_before_any_launch():
    from evacx._lib import lib
    from evacx.qmlp import evx_qmlp_grads, evx_qmlp_params, td_opts
    L = lib()
    # a NULL Q
    rc = _td_loss_opt(L, None)
    assert rc < 0 and b"NULL" in L.evx_q_last_error()
    rc = _td_loss_opt(L, td_opts(None, 0.0))
    assert rc < 0 and b"NULL" in L.evx_q_last_error()
    # a bad Huber delta is refused whatever else is passed
    for bad in (-1.0, math.nan, math.inf):
        rc = _td_loss_opt(L, td_opts(None, bad))
        assert rc == -22 and b"huber_delta" in L.evx_q_last_error(), bad
    p, g = evx_qmlp_params(), evx_qmlp_grads()

    def tdb(opt, pp):
        return L.evx_qmlp_td_backward_opt(pp, 8, None, None, None, None, None, 0.99, None, None, None, None, None, None,
                                          0.2, None, None, C.byref(g), None, None if opt is None else C.byref(opt), None)
    rc = tdb(None, C.byref(p))
    assert rc < 0 and b"NULL" in L.evx_qmlp_last_error()
    for bad in (-1.0, math.nan):
        rc = tdb(td_opts(None, bad), C.byref(p))
        assert rc == -22 and b"huber_delta" in L.evx_qmlp_last_error(), bad
    # tau outside [0, 1]
    buf = (C.c_float * 4)()
    for bad in (1.5, -0.1, math.nan):
        rc = L.evx_polyak(buf, buf, 4, bad, 0.5, None)
        assert rc == -22 and b"tau" in L.evx_q_last_error(), bad
        rc = L.evx_qmlp_polyak_pack3(buf, buf, bad, 0.5, *([None] * 10))
        assert rc == -22 and b"tau" in L.evx_qmlp_last_error(), bad
    assert L.evx_polyak(None, None, 4, 0.5, 0.5, None) == -22 and b"NULL" in L.evx_q_last_error()
    assert L.evx_qmlp_polyak_pack3(None, None, 0.5, 0.5, *([None] * 10)) == -22
    assert b"NULL" in L.evx_qmlp_last_error()


def test_validator_raises():
    from evacx.qnet import validate_td_options
    validate_td_options()
    validate_td_options("huber", 10.0, 0.005)
    validate_td_options("mse", 1, 0)
    for kw in (dict(loss="l1"), dict(loss=None), dict(huber_delta=0), dict(huber_delta=-2.0),
               dict(huber_delta=math.nan), dict(huber_delta=math.inf), dict(target_tau=1), dict(target_tau=1.0),
               dict(target_tau=-0.01), dict(target_tau=math.nan)):
        with pytest.raises(ValueError):
            validate_td_options(**kw)


def test_polyak_coefficients_are_the_f32_pair():
    import numpy as np
    from evacx.qmlp import polyak_coeffs
    for tau in (0.005, 0.37, 0.01, 0.0, 1.0):
        t, omt = polyak_coeffs(tau)
        assert t == float(np.float32(tau))
        assert omt == float(np.float32(1.0 - float(np.float32(tau))))


def test_train_vec_flags_and_config_keys():
    from Louvre_Evacuation.runners import train_vec as tv
    a = tv.parse_args([])
    assert (a.double_q, a.loss, a.huber_delta, a.target_tau) == (None, None, None, None)
    off = dict(double_q=False, loss="mse", huber_delta=1.0, target_tau=0.0)
    assert tv.td_options(a, {}) == off
    # the reference's own agent section has none of the keys
    import os
    import yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(tv.__file__), "..", "..", "configs", "dqn.yaml")))
    assert tv.td_options(a, cfg["agent"]) == off
    # the config's optional keys override the defaults ...
    keys = dict(double_dqn=True, loss="huber", huber_delta=5, target_tau=0.005)
    assert tv.td_options(a, keys) == dict(double_q=True, loss="huber", huber_delta=5.0, target_tau=0.005)
    # ... and a flag overrides the config
    a = tv.parse_args(["--double-q", "--loss", "huber", "--huber-delta", "10", "--target-tau", "0.01"])
    assert tv.td_options(a, {}) == dict(double_q=True, loss="huber", huber_delta=10.0, target_tau=0.01)
    a = tv.parse_args(["--no-double-q", "--loss", "mse", "--target-tau", "0"])
    assert tv.td_options(a, keys) == dict(double_q=False, loss="mse", huber_delta=5.0, target_tau=0.0)
    with pytest.raises(SystemExit):
        tv.parse_args(["--loss", "l1"])
    with pytest.raises(ValueError):
        tv.td_options(tv.parse_args(["--target-tau", "1"]), {})
    with pytest.raises(ValueError):
        tv.td_options(tv.parse_args([]), dict(huber_delta=0))
