"""ctypes binding of libevacx.so: the one Python description of include/evacx.h.

The structures, the mirrored constants and ``SIGNATURES`` (every entry point's return and
argument types) live here and nowhere else; tests/test_abi.py checks all three against the
header. ``lib()`` loads the library once and binds every symbol of the table, ``check`` turns a
return code into an ``EvacxError`` with the library's error text.

The library is built in-tree by ``make -C dqn-marl_amd/csrc`` (or
``__graft_entry__.build()``). There is no fallback: if it is missing or a call
fails, an ``EvacxError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# EVACX_LIB selects another in-tree build (e.g. libevacx_prof.so, the diagnostic one); EVX_LIB any
# path (experiment and older builds, tools/). An older build may lack newer symbols -- lib() skips
# them and the call sites that can do without check hasattr -- and keeps one error text per family:
# check() then shows a stale text for failures outside the env family (fine for A/B runs).
LIB_PATH = os.environ.get("EVX_LIB") or os.path.join(HERE, os.environ.get("EVACX_LIB", "libevacx.so"))


class EvacxError(RuntimeError):
    pass


# ---------------------------------------------------------------- constants (#define in the header)
FEAT_PAD = 6  # EVX_FEAT_PAD
NSTEP_MAX = 32  # EVX_NSTEP_MAX
OBS_WORDS = 8  # sizeof(evx_obs) / 4
PREC = {"f32": 0, "bf16": 1, "x3": 2}  # EVX_PREC_*
RELU, ACCUM, SPLIT_AB, OUT_SPLIT = 1, 2, 4, 8  # EVX_GEMM_*
CONV_FWD, CONV_DX, CONV_DW = 1, 2, 3  # EVX_CONV_*
# EVX_ROUTE_*: the kernel a GEMM / conv descriptor runs on (evx_gemm_plan_query)
ROUTE = {"NONE": 0, "GEMM128_F32": 1, "GEMM128_BF16": 2, "X3_VEC_AB": 3, "X3_VEC_A": 4, "X3_VEC_B": 5,
         "X3_SCALAR": 6, "X3_SPLIT_AB": 7, "TN3_KMAJOR": 8, "TN3_AK": 9, "TN3_CONV_DW": 10, "X3_CONV_FWD": 11,
         "X3_CONV_DX": 12, "X3_CONV_DW": 13, "CONV_LDS16_FWD": 14, "CONV_WREG32_FWD": 15, "CONV_LDS64_FWD": 16,
         "CONV_LDS64_DX": 17, "CONV_LDS128_DX": 18}
REDUCE = {"NONE": 0, "GENERIC": 1, "QUARTERS": 2}  # EVX_REDUCE_*: the split-K reduction kernel
# EVX_FWD_*: what an MLP forward or act call launches (evx_qmlp_fwd_plan_query, evx_qmlp_act_plan_query)
FWD = {"NONE": 0, "FC": 1, "FC_GROUPED": 2, "PAIRED": 3, "TARGET_ACT_TABLE": 4, "TARGET_ACT_FC": 5, "ACT_BF16": 6,
       "ACT_64": 7, "ACT_PERSISTENT": 8, "ACT_GROUPED": 9}
FWD_ACT_GROUPED_BLOCKED = 10  # EVX_FWD_ACT_GROUPED_BLOCKED (an enumerator): evx_qmlp_act_gb's route
EPISODE_REDUCE_SPAN = 1024  # EVX_EPISODE_REDUCE_SPAN: envs one pass of a reduce workgroup covers
EPISODE_ROW_WORDS = 10  # sizeof(evx_episode_row) / 8
HEALTH_ROW_WORDS = 6  # sizeof(evx_health_row) / 8
HEALTH_MAX_P = 16383  # EVX_HEALTH_MAX_P
LSTATS_MAX_A = 8  # EVX_LSTATS_MAX_A
LSTATS_TD_BUCKETS = 48  # EVX_LSTATS_TD_BUCKETS
LSTATS_WS_FIELDS = 10  # EVX_LSTATS_WS_FIELDS
VPROBE_ROW_WORDS = 12  # sizeof(evx_vprobe_row) / 8
SPATIAL = {"LDS": 1, "BANDS": 2}  # EVX_SPATIAL_*: how evx_spatial_update counts the dense maps
SPATIAL_MAX_GRID = 4096  # the largest GX, GY evx_spatial_update takes


# ---------------------------------------------------------------- structures
def _ptrs(*names):
    return [(n, C.c_void_p) for n in names]


class evx_layout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["L", "W", "P", "R", "t_max", "ox0", "oy0", "OX", "OY", "exit_x",
                                        "exit_y", "rx_lo", "rx_hi", "reset_view_x", "reset_view_y",
                                        "reset_robots", "flags", "repel_d2", "pad0"]] + \
               [(n, C.c_double) for n in ["repel_k", "repel_range", "evac_reward", "death_penalty",
                                         "death_acc_penalty", "alive_bonus"]] + \
               _ptrs("floor", "cellinfo", "valid_bits", "danger_p", "danger_o", "danger_o32", "robot_init",
                     "nbr_valid", "floor_d5", "obs_feat", "layout_set", "obs_feats", "obs_feat_lo", "obs_feats_lo")


class evx_state(C.Structure):
    _fields_ = [("E", C.c_int32)] + _ptrs("pk", "health", "acc", "rmap", "thmap", "robots", "view", "scal",
                                          "py_mt", "np_mt", "scratch", "order", "layout_idx", "perm_ws")


class evx_replay(C.Structure):
    _fields_ = [("capacity", C.c_int64)] + _ptrs("s", "s2", "a", "r", "done")


class evx_step_out(C.Structure):
    _fields_ = _ptrs("reward", "done", "counts", "obs", "err", "stamps", "obs_term")


class evx_env_step_plan(C.Structure):
    """How a step is launched (evx_env_step_plan_query): env_step_kernel<nwb, multi, bigg>, its LDS,
    the heavy-env path and the three LDS layout switches."""
    _fields_ = [(n, C.c_int32) for n in ["nwb", "bigg", "multi", "hcap", "hmin", "lds_env_bytes", "lds_wg_bytes",
                                        "vac_in_ring", "near_in_misc", "wide_past_envs"]]


class evx_gemm_desc(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("precision", C.c_int32),
                ("flags", C.c_int32), ("alpha", C.c_float),
                ("A", C.c_void_p), ("sam", C.c_int64), ("sak", C.c_int64),
                ("B", C.c_void_p), ("sbk", C.c_int64), ("sbn", C.c_int64),
                ("C", C.c_void_p), ("ldc", C.c_int64), ("bias", C.c_void_p),
                ("mask", C.c_void_p), ("ldm", C.c_int64), ("mask_scale", C.c_float),
                ("gate", C.c_void_p), ("ldg", C.c_int64), ("ws", C.c_void_p), ("ws_elems", C.c_int64)]


class evx_gemm_plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["route", "slices", "klen", "reduce"]]


class evx_adam(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("step", C.c_int64)]


class evx_prio(C.Structure):
    _fields_ = [("capacity", C.c_int64)] + _ptrs("sum", "mn", "max_leaf", "owner")


class evx_qmlp_params(C.Structure):
    _fields_ = _ptrs("w1", "b1c", "w2", "w2t", "b2", "w3", "b3", "w1o", "stat") + \
        [("stat_fs", C.c_int32), ("x3", C.c_int32)] + _ptrs("w1l", "w2l", "w2tl", "w1ol") + \
        [("stat_x0", C.c_int32), ("stat_nx", C.c_int32), ("stat_xin", C.c_void_p)]


class evx_qmlp_dropout(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("stream", C.c_uint32), ("p", C.c_float), ("row0", C.c_uint32),
                ("mask", C.c_void_p)]


class evx_qmlp_fwd_out(C.Structure):
    _fields_ = _ptrs("h1", "x", "h2", "q", "actions") + \
        [("epsilon", C.c_float), ("act_seed", C.c_uint64), ("act_offset", C.c_uint64), ("perm", C.c_void_p),
         ("rows_per_env", C.c_int32), ("act_ws", C.c_void_p)]


class evx_qmlp_grads(C.Structure):
    _fields_ = _ptrs("w1", "b1", "w2", "b2", "w3", "b3", "part")


class evx_td_opts(C.Structure):
    """TD options (include/evacx.h): sel = the bootstrap action per row (Double-Q; NULL: the
    target's maximum), huber_delta (0: squared error), gamma_row = the discount per row (n-step
    rows; NULL: the scalar gamma)."""
    _fields_ = [("sel", C.c_void_p), ("huber_delta", C.c_float), ("gamma_row", C.c_void_p)]


class evx_qmlp_plan(C.Structure):
    """The grouped learn chain's launch shape at B rows per net (evx_qmlp_group_plan)."""
    _fields_ = [(n, C.c_int32) for n in ["fc1_rows", "qbwd3_rows", "dw1_kper", "dw1_gz", "dw2_kper", "dw2_gz",
                                        "qdz1_tiles", "td_blocks"]]


class evx_qmlp_fwd_plan(C.Structure):
    """Every launch of one MLP forward or act call (evx_qmlp_fwd_plan_query, evx_qmlp_act_plan_query)."""
    _fields_ = [(n, C.c_int32) for n in ["route", "fc1_rows", "fc1_cols", "fc23_rows", "drop_mode", "drop_mode1",
                                        "x_expand", "act_grid", "rest_grid", "rest_listed"]]


class evx_episodes(C.Structure):
    _fields_ = [("E", C.c_int32), ("tab_slots", C.c_int32)] + \
        _ptrs("ret", "len", "w_n", "w_len", "w_evac", "w_dead", "w_ret", "w_ret2", "w_min", "w_max", "last_ret",
              "last_len", "last_evac", "last_dead", "n_total", "tab_ret", "tab_len", "tab_evac", "tab_dead")


class evx_health(C.Structure):
    _fields_ = [("E", C.c_int32), ("tab_slots", C.c_int32)] + \
        _ptrs("n_total", "w_n", "w_has", "w_alive", "w_avg", "w_min", "w_lo", "last_avg", "last_min", "last_alive",
              "tab_avg", "tab_min", "tab_alive")


class evx_timeline(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["E", "T", "n_rows", "n_trk"]] + \
        _ptrs("t", "p_evac", "p_dead", "n_total", "evac", "dead", "ended", "seen", "alive", "health_q", "late",
              "bad_health", "trk_env", "trk_person", "trk_pk", "trk_health", "trk_len")


class evx_spatial(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["E", "P", "R", "GX", "GY", "n_rows"]] + \
        _ptrs("prev", "n_total", "arrive", "stall", "evac", "died", "robot", "steps", "bad")


class evx_spatial_launch(C.Structure):
    """The launch shape of evx_spatial_update (evx_spatial_plan)."""
    _fields_ = [(n, C.c_int32) for n in ["route", "bands", "band_w", "band_cells", "lds_bytes", "envs_per_wg",
                                        "threads", "launches"]]


class evx_lstats(C.Structure):
    _fields_ = [("nets", C.c_int32), ("A", C.c_int32)] + \
        _ptrs("steps", "steps_bad", "rows", "rows_bad", "n_done", "n_greedy", "n_clipped", "act_hist", "td_hist",
              "s_q", "s_qmax", "s_y", "s_d", "s_absd", "s_d2", "s_rew", "s_loss", "s_norm",
              "max_absd", "max_q", "min_q", "max_loss", "max_norm")


class evx_vprobe(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["E", "R", "A", "pad0"]] + \
        _ptrs("open", "q0", "g", "disc", "len", "w_n", "w_bad", "w_q", "w_g", "w_e", "w_e2", "w_q2", "w_g2", "w_qg",
              "w_emin", "w_emax")


class evx_member_buf(C.Structure):
    """One [members][...] array of evx_copy_members: member k's block is bytes [0, bytes) at
    base + k * stride_bytes."""
    _fields_ = [("base", C.c_void_p), ("stride_bytes", C.c_int64), ("bytes", C.c_int64)]


# ---------------------------------------------------------------- signatures
# symbol -> (restype, argtypes), one entry per prototype of the header, in its order. A pointer to a
# structure mirrored above is typed; _vp is a `void *` (streams) or a plain data pointer (device and
# host arrays, evx_obs rows), passed as an integer address or None.
_P, _vp = C.POINTER, C.c_void_p
_i32, _i64, _u64, _f32, _f64 = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
_LAY, _ST, _RING, _PAR = _P(evx_layout), _P(evx_state), _P(evx_replay), _P(evx_qmlp_params)
_NET = [_PAR, _P(evx_qmlp_dropout), _P(evx_qmlp_fwd_out)]  # one net of a forward: params, dropout, outputs
_GRADS, _OPTS = _P(evx_qmlp_grads), _P(evx_td_opts)

SIGNATURES = {
    "evx_env_step": (C.c_int, [_LAY, _ST, _vp, _P(evx_step_out), _vp]),
    "evx_env_step_part": (C.c_int, [_LAY, _ST, _vp, _P(evx_step_out), _i32, _vp]),
    "evx_env_step_occupancy": (C.c_int, [_LAY, _ST] + [_P(_i32)] * 3),
    "evx_env_step_plan_query": (C.c_int, [_LAY, _ST, _i32, _P(evx_env_step_plan)]),
    "evx_env_reset": (C.c_int, [_LAY, _ST] + [_vp] * 4),
    "evx_obs_expand_f32": (C.c_int, [_LAY, _vp, _i64, _vp, _vp]),
    "evx_obs_expand_f64": (C.c_int, [_LAY, _vp, _i64, _vp, _vp]),
    "evx_seed_host": (C.c_int, [_vp, _i32, _vp, _vp]),
    "evx_env_order": (C.c_int, [_LAY, _ST, _vp]),
    "evx_act_perm": (C.c_int, [_LAY, _ST, _vp, _vp]),
    "evx_env_orders": (C.c_int, [_LAY, _ST, _vp, _vp]),
    "evx_env_classes": (C.c_int, [_LAY, _ST, _vp]),
    "evx_perm_ws_bytes": (C.c_int64, [_i32]),
    "evx_step_lds_bytes": (C.c_int64, [_LAY]),
    "evx_step_scratch_words": (C.c_int64, [_LAY]),
    "evx_diag_sort_keys": (C.c_int, [_vp, _vp, _i32, _vp]),
    "evx_last_error": (C.c_char_p, []),
    "evx_gemm": (C.c_int, [_P(evx_gemm_desc), _vp]),
    "evx_gemm_ws_elems": (C.c_int64, [_P(evx_gemm_desc)]),
    "evx_conv3x3_gemm": (C.c_int, [_P(evx_gemm_desc), _i32, _i32, _vp]),
    "evx_conv3x3_ws_elems": (C.c_int64, [_P(evx_gemm_desc), _i32, _i32]),
    "evx_gemm_plan_query": (C.c_int, [_P(evx_gemm_desc), _i32, _i32, _P(evx_gemm_plan)]),
    "evx_colsum": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp]),
    "evx_td_loss_ws_floats": (C.c_int64, [_i32, _i32]),
    "evx_td_loss": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32] + [_vp] * 3 + [_i64, _vp]),
    "evx_td_loss_w": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32] + [_vp] * 5 + [_i64, _vp]),
    "evx_td_loss_zero": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32] + [_vp] * 5 + [_i64, _vp, _i64, _vp]),
    "evx_sumsq_norm": (C.c_int, [_vp, _i64, _vp, _i32, _vp, _vp]),
    "evx_clip_adam": (C.c_int, [_vp] * 4 + [_i64, _vp, _f32, _P(evx_adam), _vp]),
    "evx_dropout_mask": (C.c_int, [_vp, _i64, _f32, _u64, _u64, _vp]),
    "evx_act": (C.c_int, [_vp, _i32, _i32, _f32, _u64, _u64, _vp, _vp]),
    "evx_replay_push": (C.c_int, [_RING] + [_vp] * 5 + [_i32, _i32, _i64, _vp]),
    "evx_replay_push_term": (C.c_int, [_RING] + [_vp] * 6 + [_i32, _i32, _i64, _vp]),
    "evx_env_orders_push": (C.c_int, [_LAY, _ST, _vp, _RING] + [_vp] * 6 + [_i32, _i32, _i64, _vp]),
    "evx_env_orders_push_sample": (C.c_int, [_LAY, _ST, _vp, _RING] + [_vp] * 6 +
                                   [_i32, _i32, _i64, _i32, _i64, _u64, _u64] + [_vp] * 6),
    "evx_replay_sample": (C.c_int, [_RING, _i64, _i32, _u64, _u64] + [_vp] * 7),
    "evx_replay_sample_window": (C.c_int, [_RING, _i64, _i64, _i32, _u64, _u64] + [_vp] * 7),
    "evx_replay_sample_agents": (C.c_int, [_RING, _i64, _i32, _i32, _u64, _u64] + [_vp] * 6),
    "evx_replay_sample_joint": (C.c_int, [_RING, _i64, _i32, _i32, _u64, _u64] + [_vp] * 6),
    "evx_replay_nstep": (C.c_int, [_RING, _vp, _i32] + [_i64] * 3 + [_i32, _f32] + [_vp] * 6),
    "evx_replay_sample_nstep_agents": (C.c_int, [_RING, _i64, _i32, _i32, _i32, _u64, _u64] + [_i64] * 3 +
                                       [_i32, _f32] + [_vp] * 9),
    "evx_prio_init": (C.c_int, [_P(evx_prio), _vp]),
    "evx_prio_set_range": (C.c_int, [_P(evx_prio)] + [_i64] * 3 + [_vp]),
    "evx_prio_update": (C.c_int, [_P(evx_prio), _vp, _vp, _i32, _f64, _f64, _vp]),
    "evx_prio_sample": (C.c_int, [_RING, _P(evx_prio), _i32, _f64, _u64, _u64] + [_vp] * 8),
    "evx_prio_last_error": (C.c_char_p, []),
    "evx_floor_field": (C.c_int, [_i32] * 3 + [_vp] * 6),
    "evx_floor_last_error": (C.c_char_p, []),
    "evx_gather_obs": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "evx_im2col3x3": (C.c_int, [_vp] + [_i32] * 3 + [_vp, _vp]),
    "evx_col2im3x3": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "evx_pix_split": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "evx_pix_nchw": (C.c_int, [_vp] + [_i32] * 3 + [_vp, _vp]),
    "evx_relu_grad": (C.c_int, [_vp, _vp, _i64, _vp]),
    "evx_q_last_error": (C.c_char_p, []),
    "evx_qmlp_act_ws_ints": (C.c_int64, [_i32]),
    "evx_qmlp_pack": (C.c_int, [_vp] * 9),
    "evx_qmlp_pack3": (C.c_int, [_vp] * 11),
    "evx_qmlp_pack_occ3": (C.c_int, [_vp] * 4),
    "evx_qmlp_stat": (C.c_int, [_LAY, _vp, _i32, _PAR, _vp, _vp]),
    "evx_qmlp_expand_x3": (C.c_int, [_LAY, _vp, _i32, _vp, _vp]),
    "evx_qmlp_stat_x": (C.c_int, [_LAY, _vp, _vp, _i32, _PAR, _vp, _vp]),
    "evx_qmlp_forward": (C.c_int, [_LAY, _vp, _i32, *_NET, _vp]),
    "evx_qmlp_act": (C.c_int, [_LAY, _vp, _i32, *_NET, _vp]),
    "evx_qmlp_act64": (C.c_int, [_LAY, _vp, _i32, *_NET, _vp]),
    "evx_qmlp_forward2": (C.c_int, [_LAY, _i32, _vp, *_NET, _vp, *_NET, _vp]),
    "evx_qmlp_backward_part_floats": (C.c_int64, [_i32]),
    "evx_qmlp_backward": (C.c_int, [_PAR, _i32] + [_vp] * 4 + [_f32, _vp, _vp, _GRADS, _i32, _vp]),
    "evx_qmlp_backward_ss": (C.c_int, [_PAR, _i32] + [_vp] * 4 + [_f32, _vp, _vp, _GRADS, _i32, _vp, _vp]),
    "evx_qmlp_td_backward_ss": (C.c_int, [_PAR, _i32] + [_vp] * 5 + [_f32] + [_vp] * 6 +
                                [_f32, _vp, _vp, _GRADS, _vp, _vp]),
    "evx_qmlp_norm_parts": (C.c_int32, []),
    "evx_qmlp_nparams": (C.c_int64, []),
    "evx_qmlp_sumsq_parts": (C.c_int, [_vp] * 3),
    "evx_qmlp_adam_pack3": (C.c_int, [_vp] * 4 + [_f32, _P(evx_adam)] + [_vp] * 10 + [_i32, _vp, _vp]),
    "evx_qmlp_last_error": (C.c_char_p, []),
    "evx_qmlp_act_g": (C.c_int, [_LAY, _vp, _i32, _i32, *_NET, _vp]),
    "evx_qmlp_forward2_g": (C.c_int, [_LAY, _i32, _i32, _vp, *_NET, _vp, *_NET, _vp]),
    "evx_td_loss_zero_g": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32, _i32] + [_vp] * 5 +
                           [_i64, _vp, _i64, _vp]),
    "evx_td_loss_opt": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32, _i32] + [_vp] * 5 +
                        [_i64, _vp, _i64, _OPTS, _vp]),
    "evx_qmlp_td_backward_opt": (C.c_int, [_PAR, _i32] + [_vp] * 5 + [_f32] + [_vp] * 6 +
                                 [_f32, _vp, _vp, _GRADS, _vp, _OPTS, _vp]),
    "evx_polyak": (C.c_int, [_vp, _vp, _i64, _f32, _f32, _vp]),
    "evx_qmlp_polyak_pack3": (C.c_int, [_vp, _vp, _f32, _f32] + [_vp] * 10),
    "evx_qmlp_backward_ss_g": (C.c_int, [_PAR, _i32, _i32] + [_vp] * 4 + [_f32, _vp, _vp, _GRADS, _vp, _vp]),
    "evx_qmlp_adam_pack3_g": (C.c_int, [_vp] * 4 + [_f32, _P(evx_adam)] + [_vp] * 10 + [_i32, _vp, _i32, _vp]),
    "evx_qmlp_adam_pack3_gl": (C.c_int, [_vp] * 4 + [_f32, _P(evx_adam)] + [_vp] * 10 + [_i32, _vp, _i32, _vp, _vp]),
    "evx_qmlp_group_plan": (C.c_int, [_i32, _i32, _P(evx_qmlp_plan)]),
    "evx_qmlp_fwd_plan_query": (C.c_int, [_LAY, _i32, _vp, *_NET, _vp, *_NET, _i32, _P(evx_qmlp_fwd_plan)]),
    "evx_qmlp_act_plan_query": (C.c_int, [_LAY, _vp, _i32, *_NET, _i32, _i32, _i32, _P(evx_qmlp_fwd_plan)]),
    "evx_qmlp_act_gb": (C.c_int, [_LAY, _vp, _i32, _i32, *_NET, _vp, _vp]),
    "evx_qmlp_act_gb_plan_query": (C.c_int, [_LAY, _vp, _i32, _i32, *_NET, _vp, _P(evx_qmlp_fwd_plan)]),
    "evx_replay_push_blocks": (C.c_int, [_RING] + [_vp] * 6 + [_i32, _i32, _i32, _i64, _vp]),
    "evx_replay_sample_blocks": (C.c_int, [_RING, _i64, _i32, _i32, _u64, _u64] + [_vp] * 6),
    "evx_replay_sample_nstep_blocks": (C.c_int, [_RING, _i64, _i32, _i32, _u64, _u64] + [_i64] * 3 + [_vp] * 11),
    "evx_td_loss_opt_nets": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32, _i32] + [_vp] * 5 +
                             [_i64, _vp, _i64, _OPTS, _vp, _vp]),
    "evx_qmlp_polyak_pack3_g": (C.c_int, [_vp] * 13 + [_i32, _vp]),
    "evx_copy_members": (C.c_int, [_P(evx_member_buf), _i32, _P(_i32), _i32, _vp]),
    "evx_qmix_nparams": (C.c_int32, [_i32]),
    "evx_qmix_part_floats": (C.c_int64, [_i32, _i32]),
    "evx_qmix_loss": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32, _i32] + [_vp] * 7 + [_i64, _vp]),
    "evx_qmix_loss_opt": (C.c_int, [_vp, _vp, _i32] + [_vp] * 3 + [_f32, _i32, _i32] + [_vp] * 7 +
                          [_i64, _OPTS, _vp, _vp]),
    "evx_qmix_last_error": (C.c_char_p, []),
    "evx_episode_init": (C.c_int, [_P(evx_episodes), _vp]),
    "evx_episode_update": (C.c_int, [_P(evx_episodes)] + [_vp] * 3 + [_i64, _vp]),
    "evx_episode_discard": (C.c_int, [_P(evx_episodes), _vp, _vp]),
    "evx_episode_reduce": (C.c_int, [_P(evx_episodes), _vp, _i32, _i64, _vp, _i32, _vp]),
    "evx_episode_last_error": (C.c_char_p, []),
    "evx_health_init": (C.c_int, [_P(evx_health), _vp]),
    "evx_health_update": (C.c_int, [_P(evx_health), _vp, _vp, _i32, _vp, _i64, _vp]),
    "evx_health_reduce": (C.c_int, [_P(evx_health), _vp, _i32, _vp, _i32, _vp]),
    "evx_health_last_error": (C.c_char_p, []),
    "evx_timeline_init": (C.c_int, [_P(evx_timeline), _vp]),
    "evx_timeline_update": (C.c_int, [_P(evx_timeline)] + [_vp] * 5 + [_i32, _i64, _vp]),
    "evx_timeline_trace0": (C.c_int, [_P(evx_timeline), _vp, _vp, _i32, _vp]),
    "evx_timeline_last_error": (C.c_char_p, []),
    "evx_spatial_init": (C.c_int, [_P(evx_spatial), _vp]),
    "evx_spatial_sync": (C.c_int, [_P(evx_spatial), _vp, _vp, _vp]),
    "evx_spatial_update": (C.c_int, [_P(evx_spatial)] + [_vp] * 4 + [_i64, _vp]),
    "evx_spatial_plan": (C.c_int, [_i32] * 4 + [_P(evx_spatial_launch)]),
    "evx_spatial_last_error": (C.c_char_p, []),
    "evx_lstats_ws_doubles": (C.c_int64, [_i32, _i32]),
    "evx_lstats_init": (C.c_int, [_P(evx_lstats), _vp]),
    "evx_lstats_update": (C.c_int, [_P(evx_lstats)] + [_vp] * 5 + [_f32, _i32, _OPTS, _vp, _vp, _f32, _vp, _vp, _i64,
                                                                   _vp]),
    "evx_lstats_last_error": (C.c_char_p, []),
    "evx_vprobe_init": (C.c_int, [_P(evx_vprobe), _vp]),
    "evx_vprobe_update": (C.c_int, [_P(evx_vprobe)] + [_vp] * 4 + [_f64, _vp]),
    "evx_vprobe_discard": (C.c_int, [_P(evx_vprobe), _vp, _vp]),
    "evx_vprobe_reduce": (C.c_int, [_P(evx_vprobe), _vp, _i32, _vp, _i32, _vp]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EvacxError(f"{LIB_PATH} not built: run `make -C dqn-marl_amd/csrc` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name, None)  # None: an older build under EVX_LIB that lacks the symbol
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise EvacxError(f"{what} failed ({rc}): {lib().evx_last_error().decode()}")
