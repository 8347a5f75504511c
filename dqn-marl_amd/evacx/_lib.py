"""ctypes binding of libevacx.so (include/evacx.h).

The library is built in-tree by ``make -C dqn-marl_amd/csrc`` (or
``__graft_entry__.build()``). There is no fallback: if it is missing or a call
fails, an ``EvacxError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# EVACX_LIB selects another in-tree build (e.g. libevacx_prof.so, the diagnostic one)
LIB_PATH = os.environ.get("EVX_LIB") or os.path.join(HERE, os.environ.get("EVACX_LIB", "libevacx.so"))  # EVX_LIB: experiment builds (tools/)


class EvacxError(RuntimeError):
    pass


class evx_layout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["L", "W", "P", "R", "t_max", "ox0", "oy0", "OX", "OY", "exit_x",
                                        "exit_y", "rx_lo", "rx_hi", "reset_view_x", "reset_view_y",
                                        "reset_robots", "flags", "repel_d2", "pad0"]] + \
               [(n, C.c_double) for n in ["repel_k", "repel_range", "evac_reward", "death_penalty",
                                         "death_acc_penalty", "alive_bonus"]] + \
               [(n, C.c_void_p) for n in ["floor", "cellinfo", "valid_bits", "danger_p", "danger_o",
                                         "danger_o32", "robot_init", "nbr_valid", "floor_d5", "obs_feat",
                                         "layout_set", "obs_feats", "obs_feat_lo", "obs_feats_lo"]]

FEAT_PAD = 6  # EVX_FEAT_PAD
NSTEP_MAX = 32  # EVX_NSTEP_MAX


class evx_state(C.Structure):
    _fields_ = [("E", C.c_int32)] + [(n, C.c_void_p) for n in
                                     ["pk", "health", "acc", "rmap", "thmap", "robots", "view", "scal",
                                      "py_mt", "np_mt", "scratch", "order", "layout_idx", "perm_ws"]]


class evx_replay(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("s", C.c_void_p), ("s2", C.c_void_p), ("a", C.c_void_p),
                ("r", C.c_void_p), ("done", C.c_void_p)]


class evx_step_out(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ["reward", "done", "counts", "obs", "err", "stamps", "obs_term"]]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EvacxError(f"{LIB_PATH} not built: run `make -C dqn-marl_amd/csrc` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        L.evx_last_error.restype = C.c_char_p
        L.evx_step_lds_bytes.restype = C.c_int64
        L.evx_step_scratch_words.restype = C.c_int64
        L.evx_step_lds_bytes.argtypes = [C.POINTER(evx_layout)]
        L.evx_step_scratch_words.argtypes = [C.POINTER(evx_layout)]
        for name in ["evx_env_step", "evx_env_reset", "evx_obs_expand_f32", "evx_obs_expand_f64",
                     "evx_seed_host", "evx_env_order"]:
            getattr(L, name).restype = C.c_int
        L.evx_env_step.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p,
                                   C.POINTER(evx_step_out), C.c_void_p]
        L.evx_env_step_part.restype = C.c_int
        L.evx_env_step_part.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p,
                                        C.POINTER(evx_step_out), C.c_int32, C.c_void_p]
        if hasattr(L, "evx_env_step_occupancy"):  # an older build under EVX_LIB (A/B runs) lacks the query
            L.evx_env_step_occupancy.restype = C.c_int
            L.evx_env_step_occupancy.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state)] + \
                [C.POINTER(C.c_int32)] * 3
        L.evx_env_reset.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
        L.evx_obs_expand_f32.argtypes = [C.POINTER(evx_layout), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.evx_obs_expand_f64.argtypes = [C.POINTER(evx_layout), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.evx_seed_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.evx_env_order.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p]
        L.evx_act_perm.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p, C.c_void_p]
        L.evx_env_orders.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p, C.c_void_p]
        L.evx_env_orders_push.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p,
                                          C.POINTER(evx_replay)] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32,
                                                                                        C.c_int64, C.c_void_p]
        L.evx_env_orders_push_sample.argtypes = ([C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p,
                                                  C.POINTER(evx_replay)] + [C.c_void_p] * 6 +
                                                 [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_uint64,
                                                  C.c_uint64] + [C.c_void_p] * 6)
        L.evx_env_classes.argtypes = [C.POINTER(evx_layout), C.POINTER(evx_state), C.c_void_p]
        L.evx_perm_ws_bytes.restype = C.c_int64
        L.evx_perm_ws_bytes.argtypes = [C.c_int32]
        if hasattr(L, "evx_replay_nstep"):  # (absent from older builds loaded through EVX_LIB for A/Bs)
            L.evx_replay_nstep.restype = C.c_int
            L.evx_replay_nstep.argtypes = [C.POINTER(evx_replay), C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                           C.c_int64, C.c_int32, C.c_float] + [C.c_void_p] * 6
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise EvacxError(f"{what} failed ({rc}): {lib().evx_last_error().decode()}")


# every C symbol include/evacx.h declares (checked by tests/test_abi.py)
EXPORTS = ["evx_env_step", "evx_env_reset", "evx_obs_expand_f32", "evx_obs_expand_f64", "evx_seed_host",
           "evx_step_lds_bytes", "evx_step_scratch_words", "evx_last_error", "evx_perm_ws_bytes",
           "evx_env_order", "evx_act_perm", "evx_env_orders", "evx_env_classes", "evx_env_orders_push", "evx_env_orders_push_sample",
           "evx_env_step_occupancy", "evx_replay_nstep",
           "evx_episode_init", "evx_episode_update", "evx_episode_discard", "evx_episode_reduce",
           "evx_episode_last_error",
           "evx_health_init", "evx_health_update", "evx_health_reduce", "evx_health_last_error"]
