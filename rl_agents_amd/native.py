"""ctypes binding of libmi355plan.so (include/mi355plan.h) -- the only compute path of this package.

There is no CPU fallback: importing works anywhere (so that host logic can be unit-tested), but
creating a :class:`Context` raises if the library is missing or no MI355X is visible.
north_star asks for a cffi ABI-mode layer; cffi is not installed in this image, ctypes binds the
same C ABI (INTEGRATION.md shows both).
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MP_MEM_HOST, MP_MEM_DEVICE, MP_MEM_RNG_DEVICE = 0, 1, 2
MP_OK, MP_ERR_HIP, MP_ERR_REWARD_RANGE, MP_ERR_ALLOC, MP_ERR_ARG, MP_ERR_MODE = 0, -1, -2, -3, -4, -5
MODE_DETERMINISTIC, MODE_STOCHASTIC, MODE_SPARSE, MODE_CARTPOLE = 0, 1, 2, 3
ERR_REWARD_RANGE, ERR_ARG, ERR_MODE = -2, -4, -5
MP_ERR_GBOPD_DIVERGED, MP_ERR_GBOPD_NO_ACTION = -7, -8
ERR_GAPE_NO_CHALLENGER = -9  # mp_gape_plan status: the root lists one action (mdp_gape.py:247 ValueError)
ERR_GAPE_PLACEHOLDERS = -10  # mp_gape_plan_stochastic status: no placeholder left for a new next state (mdp_gape.py:284 ValueError)
ERR_GBOP_PLACEHOLDERS = -11   # mp_gbop_plan status: no placeholder left for a new next state (graph_based_stochastic.py:217 ValueError)
ERR_GBOP_REWARD_THRESHOLD = -12   # mp_gbop_plan status: a nonzero reward threshold reached the mis-called kl_upper_bound (:79-82 TypeError)
ERR_GBOP_CHOICE_P = -13       # mp_gbop_plan status: p_minus fails Generator.choice's checks in get_plan (:156 ValueError)
ERR_OLOP_KEY = -6          # mp_olop_plan status: the "zeros" continuation's action is not a child (olop.py:89 KeyError)

_LIB = None

c_i32, c_i64, c_f64, c_u8, c_u64 = C.c_int32, C.c_int64, C.c_double, C.c_uint8, C.c_uint64
P = C.POINTER
_vp = C.c_void_p

# every symbol include/mi355plan.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mp_last_error": (C.c_char_p, []),
    "mp_abi_version": (C.c_int, []),
    "mp_ctx_create": (C.c_int, [C.c_int, _vp, P(_vp)]),
    "mp_ctx_destroy": (C.c_int, [_vp]),
    "mp_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "mp_ctx_synchronize": (C.c_int, [_vp]),
    "mp_ctx_device_faults": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "mp_ctx_get_stream": (C.c_int, [_vp, P(_vp)]),
    "mp_ctx_device_info": (C.c_int, [_vp, P(c_i32), P(c_i32), P(c_i64), P(c_i64), C.c_char_p, c_i32]),
    "mp_model_load_table": (C.c_int, [_vp, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, c_i32, P(_vp)]),
    "mp_model_load_table_batch": (C.c_int, [_vp, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, c_i32, P(_vp)]),
    "mp_model_batch_info": (C.c_int, [_vp, P(c_i32), P(c_i32)]),
    "mp_model_update_tables": (C.c_int, [_vp, c_i32, c_i32, _vp, _vp, _vp]),
    "mp_model_update_rows": (C.c_int, [_vp, c_i32, _vp, _vp, _vp, _vp]),
    "mp_vi_solve_batch": (C.c_int, [_vp, _vp, c_f64, c_i32, c_f64, c_f64, _vp, _vp, c_i32]),
    "mp_uct_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, _vp, c_i32, c_i32, c_f64, c_f64, _vp, _vp, _vp, c_i32, _vp, _vp,
                                     _vp, _vp, _vp, _vp, c_i32]),
    "mp_opd_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_f64, c_f64, _vp, c_i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                     c_i32]),
    "mp_comm_unique_id": (C.c_int, [_vp]),
    "mp_comm_init": (C.c_int, [_vp, c_i32, c_i32, _vp]),
    "mp_gather_results": (C.c_int, [_vp, _vp, c_i32, c_i32, _vp, _vp]),
    "mp_comm_destroy": (C.c_int, [_vp]),
    "mp_libm_sincos_variant": (C.c_int, []),
    "mp_libm_sincos": (C.c_int, [c_i32, _vp, c_i32, _vp, _vp]),
    "mp_selftest_sincos": (C.c_int, [_vp, c_i32, _vp, c_i32, _vp, _vp]),
    "mp_selftest_olop_bound": (C.c_int, [_vp, c_i32, c_i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_model_load_dense": (C.c_int, [_vp, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, P(_vp)]),
    "mp_model_load_dense_rows": (C.c_int, [_vp, c_i32, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, P(_vp)]),
    "mp_vi_backup": (C.c_int, [_vp, _vp, c_f64, c_i32, _vp, _vp, c_i32]),
    "mp_model_load_sparse": (C.c_int, [_vp, c_i32, c_i32, c_i32, _vp, _vp, _vp, _vp, P(_vp)]),
    "mp_model_load_cartpole": (C.c_int, [_vp, _vp, P(_vp)]),
    "mp_model_free": (C.c_int, [_vp]),
    "mp_model_info": (C.c_int, [_vp, P(c_i32), P(c_i32), P(c_i32), P(c_i32), P(c_i32)]),
    "mp_vi_solve": (C.c_int, [_vp, _vp, c_f64, c_i32, c_f64, c_f64, c_i32, _vp, _vp, c_i32]),
    "mp_vi_solve_v": (C.c_int, [_vp, _vp, c_f64, c_i32, c_f64, c_f64, _vp, c_i32]),
    "mp_vi_solve_v_robust": (C.c_int, [_vp, _vp, c_f64, c_i32, c_f64, c_f64, _vp, c_i32]),
    "mp_vi_sweeps": (C.c_int, [_vp, _vp, c_f64, c_i32, c_i32]),
    "mp_vi_form_names": (C.c_char_p, []),
    "mp_vi_graph_captures": (c_i64, [_vp]),
    "mp_vi_geometry": (C.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, _vp]),
    "mp_vi_batch_geometry": (C.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, _vp, P(C.c_char_p)]),
    "mp_vi_dense_mode": (C.c_int, [_vp, c_i32]),
    "mp_uct_record_visits": (C.c_int, [_vp, _vp]),
    "mp_vi_exact_plan": (C.c_int, [c_i32, c_i32, _vp, c_i32, _vp, c_i32, _vp, _vp]),
    "mp_uct_plan": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, c_f64, _vp, _vp, _vp, c_i32, _vp, _vp,
                              _vp, _vp, _vp, _vp, c_i32]),
    "mp_policy_load": (C.c_int, [_vp, _vp, _vp, _vp, P(_vp)]),
    "mp_policy_free": (C.c_int, [_vp]),
    "mp_uct_plan_policy": (C.c_int, [_vp, _vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, c_f64, _vp, c_i32, _vp, _vp,
                                     _vp, _vp, _vp, _vp, c_i32]),
    "mp_uct_step_tree": (C.c_int, [_vp, c_i32, _vp, c_i32]),
    "mp_uct_step_tree_select": (C.c_int, [_vp, c_i32, _vp, _vp, c_i32]),
    "mp_uct_reset_tree": (C.c_int, [_vp]),
    "mp_uct_tree_capacity": (C.c_int, [_vp, P(c_i32)]),
    "mp_uct_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_uct_path_count": (C.c_int, [_vp, c_i32, _vp, c_i32, P(C.c_int64)]),
    "mp_model_set_available": (C.c_int, [_vp, _vp]),
    "mp_model_set_episode_rules": (C.c_int, [_vp, c_i32, c_i32]),
    "mp_uct_plan_stochastic": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, c_f64, _vp, _vp, c_i32, _vp, _vp,
                                         c_i32, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_uct_plan_stochastic_policy": (C.c_int, [_vp, _vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, c_f64, c_i32, _vp, _vp,
                                                c_i32, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_uct_stoch_tree_priors": (C.c_int, [_vp, c_i32, _vp]),
    "mp_uct_stoch_tree_capacity": (C.c_int, [_vp, P(c_i32)]),
    "mp_uct_stoch_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp]),
    "mp_policy_load_listed": (C.c_int, [_vp, _vp, _vp, _vp, _vp, P(_vp)]),
    "mp_policy_load_ordered": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, P(_vp)]),
    "mp_policy_load_rows": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, c_i32, P(_vp)]),
    "mp_opd_plan": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_f64, c_f64, _vp, c_i32, _vp, _vp, _vp, _vp, _vp, _vp,
                              c_i32]),
    "mp_opd_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_model_load_joint": (C.c_int, [_vp, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, P(_vp)]),
    "mp_ropd_plan": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_f64, c_f64, _vp, c_i32, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_ropd_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_model_set_available_joint": (C.c_int, [_vp, _vp]),
    "mp_model_load_joint_batch": (C.c_int, [_vp, c_i32, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, P(_vp)]),
    "mp_model_update_joint_tables": (C.c_int, [_vp, c_i32, c_i32, _vp, _vp, _vp]),
    "mp_model_set_available_joint_batch": (C.c_int, [_vp, _vp]),
    "mp_ropd_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_f64, c_f64, _vp, c_i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                      c_i32]),
    "mp_saopd_create": (C.c_int, [_vp, _vp, c_i32, P(_vp)]),
    "mp_saopd_free": (C.c_int, [_vp]),
    "mp_saopd_plan": (C.c_int, [_vp, _vp, _vp, c_i32, c_f64, c_f64, c_f64, c_i32, c_i32, _vp, c_i32, _vp, _vp, _vp, _vp,
                                _vp, c_i32]),
    "mp_saopd_info": (C.c_int, [_vp, P(c_i32), P(c_i32), P(c_i32), P(c_i32)]),
    "mp_saopd_export": (C.c_int, [_vp, c_i32, c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_gbopd_create": (C.c_int, [_vp, _vp, c_i32, c_i32, P(_vp)]),
    "mp_gbopd_free": (C.c_int, [_vp]),
    "mp_gbopd_plan": (C.c_int, [_vp, _vp, _vp, c_i32, c_f64, c_f64, c_f64, c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_gbopd_info": (C.c_int, [_vp, P(c_i32), P(c_i32), P(c_i32), P(c_i32), P(c_i64)]),
    "mp_gbopd_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, P(c_i64), P(c_i32)]),
    "mp_olop_allocation": (C.c_int, [c_i32, c_f64, P(c_i32), P(c_i32)]),
    "mp_olop_plan": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_i32, c_f64, c_i32, c_i32, _vp, _vp, _vp, c_i32, _vp, _vp, _vp,
                               _vp, _vp, c_i32]),
    "mp_olop_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_olop_plan_stochastic": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_i32, c_f64, c_i32, c_i32, _vp, _vp, _vp, c_i32, _vp, _vp,
                                          _vp, _vp, _vp, c_i32]),
    "mp_olop_stoch_form_names": (C.c_char_p, []),
    "mp_gape_plan": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_i32, c_f64, c_f64, c_i32, c_i32, _vp, _vp, _vp, _vp, c_i32, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_gape_form_names": (C.c_char_p, []),
    "mp_gape_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, c_f64, c_i32, c_i32, _vp, _vp, _vp, _vp, c_i32,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_gape_each_form_names": (C.c_char_p, []),
    "mp_gape_each_form_info": (C.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, _vp]),
    "mp_gape_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_gape_plan_stochastic": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_i32, c_i32, c_f64, c_f64, c_i32, c_i32, _vp, _vp, _vp, _vp,
                                          _vp, c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_gape_stoch_form_names": (C.c_char_p, []),
    "mp_gape_plan_stochastic_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_i32, c_f64, c_f64, c_i32, c_i32, _vp, _vp,
                                                 _vp, _vp, _vp, c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_gape_stoch_each_form_names": (C.c_char_p, []),
    "mp_gape_stoch_each_form_info": (C.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, _vp]),
    "mp_gbop_create": (C.c_int, [_vp, _vp, c_i32, c_i32, c_i32, P(_vp)]),
    "mp_gbop_free": (C.c_int, [_vp]),
    "mp_gbop_plan": (C.c_int, [_vp, _vp, _vp, c_i32, c_i32, c_i32, c_f64, c_f64, c_f64, c_i32, c_i32, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_gbop_info": (C.c_int, [_vp, P(c_i32), P(c_i32), P(c_i32), P(c_i32), P(c_i32), P(c_i64), P(c_i64)]),
    "mp_gbop_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32)] + [_vp] * 20 + [P(c_i64), P(c_i32)]),
    "mp_gbop_form_names": (C.c_char_p, []),
    "mp_gape_stoch_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_selftest_gape_transition": (C.c_int, [_vp, c_i32, c_i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_brue_plan":(C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_i32, c_f64, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_brue_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_olop_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, c_i32, c_i32, _vp, _vp, _vp, c_i32, _vp, _vp,
                                      _vp, _vp, _vp, c_i32]),
    "mp_brue_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, _vp, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_each_form_info": (C.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, _vp]),
    "mp_each_form_names": (C.c_char_p, []),
    "mp_ss_plan": (C.c_int, [_vp, _vp, c_i32, _vp, c_i32, c_i32, c_f64, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_ss_tree_export": (C.c_int, [_vp, c_i32, c_i32, P(c_i32), _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_ss_geometry": (C.c_int, [c_i32, c_i32, c_i32, c_i32, _vp]),
    "mp_ss_form_names": (C.c_char_p, []),
    "mp_ss_plan_models": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, c_i32, c_i32, c_f64, _vp, _vp, _vp, _vp, _vp, c_i32]),
    "mp_ss_each_form_names": (C.c_char_p, []),
    "mp_uct_choose_form": (C.c_int, [_vp, _vp, P(C.c_char_p)]),
    "mp_saopd_choose_form": (C.c_int, [_vp, _vp, P(C.c_char_p), P(C.c_char_p)]),
    "mp_last_kernel_ms": (C.c_int, [_vp, P(c_f64), P(c_i32)]),
    "mp_last_kernel_variant": (C.c_char_p, [_vp]),
    "mp_uct_last_action_table": (C.c_int, [_vp]),
    "mp_kernel_form_names": (C.c_char_p, []),
    "mp_selftest_lds_atomic_order": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64)]),
    "mp_env_step": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, _vp, _vp, c_i32, c_i32, _vp, _vp, _vp, _vp, c_i32, _vp, c_i32]),
    "mp_greedy_actions": (C.c_int, [_vp, c_i32, c_i32, c_i32, _vp, _vp, _vp, c_i32, c_i32]),
    "mp_env_step_stochastic": (C.c_int, [_vp, _vp, c_i32, _vp, _vp, _vp, _vp, c_i32, c_i32, _vp, _vp, _vp, _vp, c_i32, _vp, _vp,
                                         c_i32]),
    "mp_host_alloc": (C.c_int, [_vp, c_i64, P(_vp)]),
    "mp_host_free": (C.c_int, [_vp, _vp]),
    "mp_rng_create": (C.c_int, [_vp, c_i32, P(_vp)]),
    "mp_rng_free": (C.c_int, [_vp]),
    "mp_rng_set": (C.c_int, [_vp, c_i32, c_i32, _vp]),
    "mp_rng_get": (C.c_int, [_vp, c_i32, c_i32, _vp]),
    "mp_rng_seed_sequence": (C.c_int, [_vp, c_i32, c_i32, _vp, c_i32, c_i64]),
    "mp_rng_device_ptr": (_vp, [_vp, c_i32]),
    "mp_seed_sequence_states": (C.c_int, [_vp, c_i32, c_i64, c_i32, _vp]),
    "mp_pack_rows": (C.c_int, [_vp, _vp, c_i32, c_i32, c_i32, _vp, _vp, _vp]),
    "mp_unpack_rows": (C.c_int, [_vp, _vp, c_i32, c_i32, c_i32, c_i32, _vp, _vp, _vp]),
}


class CartPoleParams(C.Structure):
    _fields_ = [("gravity", c_f64), ("masscart", c_f64), ("masspole", c_f64), ("length", c_f64),
                ("force_mag", c_f64), ("tau", c_f64), ("theta_threshold", c_f64), ("x_threshold", c_f64),
                ("max_steps", c_i32), ("euler", c_i32)]


class NativeError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libmi355plan error {}: {}".format(code, message))
        self.code = code


def lib_path():
    """The in-tree library; MI355PLAN_LIB points at another build of the same sources (kernel A/B experiments)."""
    return os.environ.get("MI355PLAN_LIB") or _build.LIB_PATH


def _bind_torch_hip_runtime():
    """One HIP runtime per process: when PyTorch is installed, libmi355plan.so must bind to the copy of libamdhip64 that torch
    ships (streams, events and device pointers then cross freely between the two).  Rounds 1-5 got that by importing torch before
    loading the library -- 0.55 s of the first act() of a process that never uses torch (profiles/r06_first_act.txt).  Now: if
    torch is already imported, nothing to do; else torch's libamdhip64 is loaded BY PATH (importlib finds the package without
    importing it), so the library binds to it and a later `import torch` finds its runtime already in the process.
    MI355PLAN_EAGER_TORCH=1 restores the import."""
    import sys
    if "torch" in sys.modules:
        return
    if os.environ.get("MI355PLAN_EAGER_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the C ABI itself
            pass
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        for root in (list(spec.submodule_search_locations) if spec is not None and spec.submodule_search_locations else []):
            cand = os.path.join(root, "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
                return
    except Exception:  # pragma: no cover - no torch, or an unusual layout: the library then loads the system runtime
        pass


def load():
    """Load libmi355plan.so; raises (never falls back) if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError("{} is missing: run `python -m rl_agents_amd.build` (hipcc, gfx950). "
                           "There is no CPU fallback for the planning kernels.".format(path))
    if not os.environ.get("MI355PLAN_NO_TORCH"):
        _bind_torch_hip_runtime()
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.mp_abi_version() != 7:
        raise RuntimeError("libmi355plan ABI version mismatch")
    _LIB = lib
    return lib


def _check(rc):
    if rc != 0:
        raise NativeError(rc, load().mp_last_error().decode("utf-8", "replace"))


def _ptr(a):
    """numpy array / torch tensor / None -> void* address."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    raise TypeError("expected numpy array, torch tensor or None, got {}".format(type(a)))


def _ptrs(*arrays):
    return [_ptr(a) for a in arrays]


def _check_rng(rng_state, n, shape="n_roots", or_what=""):
    """The generator records of a host-array call are a C-contiguous uint64 array of ``n`` records, or ValueError."""
    if not (isinstance(rng_state, np.ndarray) and rng_state.dtype == np.uint64 and rng_state.flags.c_contiguous
            and rng_state.size == n * 6):
        raise ValueError("rng_state must be a C-contiguous uint64 array of shape [{}, 6]{}".format(shape, or_what))


# The result arrays of every planner family, in the order of the C arguments: (name, dtype, trailing shape, fill), a
# trailing "L" = the plan length, "A" = the model's actions.  The host result dicts, plan_buffers and the pinned scratch
# arrays of small plans are all made from it.
_PLANS, _LEN, _STEPS = ("plans", np.int32, ("L",), -1), ("plan_len", np.int32, (), 0), ("env_steps", np.int64, (), 0)
_ACTION, _VALUE, _STATUS = ("plans", np.int32, (), -1), ("root_value", np.float64, (), 0), ("status", np.int32, (), 0)
RESULTS = {
    "uct": (_PLANS, _LEN, _VALUE, ("root_child_count", np.int64, ("A",), 0), ("root_child_value", np.float64, ("A",), 0), _STEPS),
    "opd": (_PLANS, _LEN, ("root_lower", np.float64, (), 0), ("root_upper", np.float64, (), 0), _STEPS, _STATUS),
    "olop": (_PLANS, _LEN, _VALUE, _STEPS, _STATUS),
    "brue": (_ACTION, _VALUE, _STEPS, _STATUS),
    "gape": (_PLANS, _LEN, ("episodes_run", np.int32, (), 0), _STEPS, _STATUS, ("child_lower", np.float64, ("A",), 0),
             ("child_upper", np.float64, ("A",), 0), ("child_count", np.int64, ("A",), 0), ("best_challenger", np.int32, ("P",), -1)),
    "ss": (_ACTION, _VALUE, ("samples", np.int64, (), 0), _STATUS),
    "saopd": (_PLANS, _LEN, _STEPS, ("updates", np.int64, (), 0), _STATUS),
    "gbopd": (_PLANS, _LEN, ("value_lower", np.float64, (), 0), ("value_upper", np.float64, (), 0), _STEPS,
              ("updates", np.int64, (), 0), _STATUS),
    "gbop": (_ACTION, ("key", np.int32, (), 0), _LEN, ("value_lower", np.float64, (), 0), ("value_upper", np.float64, (), 0),
             _STEPS, ("pops", np.int64, (), 0), _STATUS),
}
# what a small plan's pinned scratch arrays hold in front of the family's results
SCRATCH_INPUTS = {"uct": (("root_state", np.int32, ()), ("root_steps", np.int32, ()), ("rng", np.uint64, (6,))),
                  "opd": (("root_state", np.int32, ()), ("rng", np.uint64, (6,)))}


def _results(family, n, **dims):
    """The host result dict of a plan of ``n`` roots."""
    out = {}
    for k, dtype, tail, fill in RESULTS[family]:
        out[k] = np.zeros((n,) + tuple([dims[d] for d in tail]) if tail else n, dtype)
        if fill:
            out[k].fill(fill)
    return out


def _result_spec(family, n, **dims):
    """``{name: (shape, dtype)}`` of the family's results (PinnedArrays' spec); an array whose dimension is None is left out."""
    return {k: ((n,) + tuple(dims[d] for d in tail), dtype) for k, dtype, tail, _ in RESULTS[family]
            if None not in [dims[d] for d in tail]}


def _result_ptrs(family, out):
    """The addresses of the result arrays ``out`` holds, in the order of the C arguments (None: not asked for)."""
    return [_ptr(out[k]) if k in out else None for k, _, _, _ in RESULTS[family]]


def _zeros(cap, fields):
    """``fields`` (name, dtype, trailing shape) -> ``{name: zeros [cap, ...]}``."""
    return {k: np.zeros((cap,) + tuple(tail), dtype) for k, dtype, tail in fields}


def _export_tree(fn, head, cap, fields):
    """A tree export ``fn(*head, cap, &n, one pointer per field)`` -> the fields' arrays, cut to the n nodes and copied."""
    t, n = _zeros(cap, fields), c_i32()
    _check(fn(*(tuple(head) + (int(cap), C.byref(n)) + tuple(_ptr(v) for v in t.values()))))
    return {k: v[:n.value].copy() for k, v in t.items()}


def _flags(x, *shape):
    """Flags (terminal, available, listed, ...) -> contiguous uint8 of ``shape`` (none: the shape they have); None stays."""
    if x is None:
        return None
    x = np.asarray(x)
    return np.ascontiguousarray((x.reshape(shape) if shape else x).astype(np.uint8))


def _same_shape(a, b, ndims, message):
    if a.shape != b.shape or a.ndim not in ndims:
        raise ValueError(message)


def _int_tables(transition, reward, ndims, message):
    """Deterministic tables as the library reads them: int64 next states and float64 rewards of one shape."""
    t = np.ascontiguousarray(transition, dtype=np.int64)
    r = np.ascontiguousarray(reward, dtype=np.float64)
    _same_shape(t, r, ndims, message)
    return t, r


def _priors(prior_p, rollout_p, n_actions=None):
    """The per-action prior / rollout probabilities as float64; ``n_actions``: the length both must have."""
    pp = np.ascontiguousarray(prior_p, dtype=np.float64)
    rp = np.ascontiguousarray(rollout_p, dtype=np.float64)
    if n_actions is not None and (pp.shape != (n_actions,) or rp.shape != (n_actions,)):
        raise ValueError("prior_p / rollout_p must have one entry per action")
    return pp, rp


class _Handle(object):
    """Owner of a library handle ``_h`` made on the context ``ctx``: ``close`` gives it to the class's ``_free`` symbol, once
    and only while the context lives; a dying owner closes itself and swallows what that raises."""
    _free = None

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            getattr(self.ctx._lib, self._free)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def entropy_words(entropy):
    """numpy's split of entropy integers into little-endian uint32 words (bit_generator.pyx _coerce_to_uint32_array):
    an int or a sequence of ints, each non-negative; 0 -> [0]."""
    ints = [entropy] if isinstance(entropy, (int, np.integer)) else list(entropy)
    words = []
    for v in ints:
        v = int(v)
        if v < 0:
            raise ValueError("expected non-negative integer")
        if v == 0:
            words.append(0)
        while v > 0:
            words.append(v & 0xFFFFFFFF)
            v >>= 32
    return np.asarray(words, dtype=np.uint32)


def seed_sequence_states(entropy, first_key, count):
    """PCG64 records uint64 [count, 6] of Generator(PCG64(SeedSequence(list(entropy) + [first_key + i]))), i < count --
    numpy's SeedSequence hashing and PCG64 seeding restated in C (mp_seed_sequence_states: host arithmetic, no GPU),
    ~1000x faster than constructing the generators in Python (262 144 roots: seconds -> milliseconds).  ``entropy``:
    int, sequence of ints, or () for SeedSequence(first_key + i)."""
    w = entropy_words(entropy) if not (hasattr(entropy, "__len__") and len(entropy) == 0) else np.zeros(0, np.uint32)
    out = np.zeros((int(count), 6), dtype=np.uint64)
    _check(load().mp_seed_sequence_states(_ptr(w) if len(w) else None, len(w), int(first_key), int(count), _ptr(out)))
    return out


def libm_sincos_variant():
    """Which restated form of glibc's small-argument sin / cos reproduces this host's libm (mp_libm_sincos_variant):
    1 = FMA-contracted, 2 = every operation rounded, 0 = neither (CartPole then keeps the device's own sincos)."""
    return int(load().mp_libm_sincos_variant())


def libm_sincos(x, variant):
    """The restated functions on the host: (sin, cos) arrays of ``x`` in form ``variant`` (0 = libm itself)."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    s, c = np.zeros_like(x), np.zeros_like(x)
    _check(load().mp_libm_sincos(int(x.size), _ptr(x), int(variant), _ptr(s), _ptr(c)))
    return s, c


def olop_allocation(budget, gamma):
    """OLOP.allocation (tree_search/olop.py:50-62): budget -> (episodes, horizon)."""
    e, h = c_i32(), c_i32()
    rc = load().mp_olop_allocation(int(budget), float(gamma), C.byref(e), C.byref(h))
    if rc != 0:
        raise ValueError("Could not split budget {} with gamma {}".format(budget, gamma))
    return e.value, h.value


UCT_CALL_FIELDS = ("n_roots", "episodes", "horizon", "A", "S", "NB", "Sb", "t16", "r8", "n_rdict", "cart", "policy", "kept_il",
                   "cus")
UCT_FORM_FIELDS = ("tree_il", "lanes", "waves", "rep_shift", "roots_per_wg", "threads", "lds")


def uct_choose_form(call):
    """The kernel form mp_uct_plan* chooses for a call (mp_uct_choose_form; host only): ``call`` holds the UCT_CALL_FIELDS in
    order, the MP_UCT_* knobs come from the environment -> (name, int64 array of the UCT_FORM_FIELDS).  A shape the plan
    refuses raises its NativeError."""
    c = np.ascontiguousarray(call, dtype=np.int64)
    assert c.shape == (len(UCT_CALL_FIELDS),), c.shape
    out = np.zeros(len(UCT_FORM_FIELDS), dtype=np.int64)
    name = C.c_char_p()
    _check(load().mp_uct_choose_form(_ptr(c), _ptr(out), C.byref(name)))
    return name.value.decode(), out


SAOPD_CALL_FIELDS = ("n", "S", "A", "budget", "n_nodes", "cap", "qcap", "have_cost", "device_arrays", "cus")
SAOPD_FORM_FIELDS = ("wave", "K", "need", "cap", "qcap", "pool_ints", "tab_plain", "tab_lds", "lds_rows", "lds_qcap", "scap",
                     "scap_global", "par_backup", "csr_old", "prune_rows", "sticky", "ordered", "lds", "lds_fallback",
                     "max_queue_bytes")


def saopd_choose_form(call):
    """The kernel form StateAwarePlanners.plan chooses for a call (mp_saopd_choose_form; host only): ``call`` holds the
    SAOPD_CALL_FIELDS in order, the MP_SAOPD_* knobs come from the environment -> (name of the first launch, name of the
    form a full backup queue falls back to, int64 array of the SAOPD_FORM_FIELDS).  Sizes the plan refuses raise its
    NativeError."""
    c = np.ascontiguousarray(call, dtype=np.int64)
    assert c.shape == (len(SAOPD_CALL_FIELDS),), c.shape
    out = np.zeros(len(SAOPD_FORM_FIELDS), dtype=np.int64)
    name, fallback = C.c_char_p(), C.c_char_p()
    _check(load().mp_saopd_choose_form(_ptr(c), _ptr(out), C.byref(name), C.byref(fallback)))
    return name.value.decode(), fallback.value.decode(), out


def kernel_form_names():
    """Every name Context.last_kernel_variant() can return (mp_kernel_form_names; host only), in the library's order."""
    return load().mp_kernel_form_names().decode().split()


def each_form_names():
    """The names OLOP and BRUE plans on one MDP per root (``olop_plan`` / ``brue_plan`` with ``model_index``) record for
    Context.last_kernel_variant() (mp_each_form_names; host only).  They are not part of kernel_form_names()."""
    return load().mp_each_form_names().decode().split()


EACH_PLANNERS = {"olop": 0, "brue": 1, "ss": 2}


def each_form_info(planner, s_each, n_actions, horizon, n_roots, cus=256):
    """The form ``olop_plan`` / ``brue_plan`` / ``ss_plan`` with ``model_index`` take for a call of this description (mp_each_form_info; host
    only, MP_EACH_MODEL is read): dict(lds_bytes = what a workgroup of the LDS form takes, lds = the call takes it, grid,
    launch_lds_bytes, default_limit = the most bytes that take the LDS form by default, fit_limit = the most that fit a compute
    unit's LDS and can be forced).  ``planner``: "olop", "brue" or "ss"."""
    out = np.zeros(6, np.int64)
    _check(load().mp_each_form_info(EACH_PLANNERS[planner], int(s_each), int(n_actions), int(horizon), int(n_roots), int(cus),
                                    _ptr(out)))
    return dict(lds_bytes=int(out[0]), lds=bool(out[1]), grid=int(out[2]), launch_lds_bytes=int(out[3]), default_limit=int(out[4]),
                fit_limit=int(out[5]))


def gape_form_names():
    """The names an MDP-GapE plan (``gape_plan``) records for Context.last_kernel_variant() (mp_gape_form_names; host only).
    They are part of no other list of names."""
    return load().mp_gape_form_names().decode().split()


def gape_each_form_names():
    """The names an MDP-GapE plan on one MDP per root (``gape_plan`` with ``model_index``) records for
    Context.last_kernel_variant() (mp_gape_each_form_names; host only).  They are part of no other list of names."""
    return load().mp_gape_each_form_names().decode().split()


def gape_each_form_info(s_each, n_actions, horizon, n_roots, cus=256):
    """The form ``gape_plan`` with ``model_index`` takes for a call of this description (mp_gape_each_form_info; host only,
    MP_EACH_MODEL is read): the dict of :func:`each_form_info`."""
    out = np.zeros(6, np.int64)
    _check(load().mp_gape_each_form_info(int(s_each), int(n_actions), int(horizon), int(n_roots), int(cus), _ptr(out)))
    return dict(lds_bytes=int(out[0]), lds=bool(out[1]), grid=int(out[2]), launch_lds_bytes=int(out[3]), default_limit=int(out[4]),
                fit_limit=int(out[5]))


def gape_stoch_form_names():
    """The names an MDP-GapE plan with transition bounds (``gape_plan_stochastic``) records for Context.last_kernel_variant()
    (mp_gape_stoch_form_names; host only).  They are part of no other list of names."""
    return load().mp_gape_stoch_form_names().decode().split()


def gape_stoch_each_form_names():
    """The names an MDP-GapE plan with transition bounds on one MDP per root (``gape_plan_stochastic_models``)
    records for Context.last_kernel_variant() (mp_gape_stoch_each_form_names; host only).  They are part of no other list."""
    return load().mp_gape_stoch_each_form_names().decode().split()


def gape_stoch_each_form_info(s_each, n_actions, horizon, n_roots, cus=256):
    """The form ``gape_plan_stochastic_models`` takes for a call of this description
    (mp_gape_stoch_each_form_info; host only, MP_EACH_MODEL is read): the dict of :func:`each_form_info`."""
    out = np.zeros(6, np.int64)
    _check(load().mp_gape_stoch_each_form_info(int(s_each), int(n_actions), int(horizon), int(n_roots), int(cus), _ptr(out)))
    return dict(lds_bytes=int(out[0]), lds=bool(out[1]), grid=int(out[2]), launch_lds_bytes=int(out[3]), default_limit=int(out[4]),
                fit_limit=int(out[5]))


def gbop_form_names():
    """The names a GBOP plan (``StochasticGraphBasedPlanners.plan``) records for Context.last_kernel_variant()
    (mp_gbop_form_names; host only).  They are part of no other list of names."""
    return load().mp_gbop_form_names().decode().split()


def olop_stoch_form_names():
    """The names an OLOP plan on a dense / sparse model (``olop_plan_stochastic``) records for
    Context.last_kernel_variant() (mp_olop_stoch_form_names; host only).  They are part of no other list of names."""
    return load().mp_olop_stoch_form_names().decode().split()


def ss_form_names():
    """The names a Sparse Sampling plan records for Context.last_kernel_variant() (mp_ss_form_names; host only).  They are
    not part of kernel_form_names()."""
    return load().mp_ss_form_names().decode().split()


def ss_each_form_names():
    """The names a Sparse Sampling plan on one MDP per root (``ss_plan`` with ``model_index``) records for
    Context.last_kernel_variant() (mp_ss_each_form_names; host only).  They are part of no other list of names."""
    return load().mp_ss_each_form_names().decode().split()


def ss_geometry(n_actions, horizon, C, W):
    """Host arithmetic of a Sparse Sampling plan (mp_ss_geometry; no device): ``W`` = the most outcomes one (state, action) can
    give -- 1 for deterministic tables, B for sparse models, the fullest row's non-zeros for dense ones.  -> dict with the
    entries of an outcome list, the bytes of a wave's frames, the node bound of a tree (-1: beyond int32 indices), the LDS
    share the frames may take by default and whether this call's frames go to LDS (MP_SS_FRAMES is read)."""
    out = np.zeros(5, np.int64)
    _check(load().mp_ss_geometry(int(n_actions), int(horizon), int(C), int(W), _ptr(out)))
    return dict(list_entries=int(out[0]), frame_bytes=int(out[1]), node_bound=int(out[2]), lds_limit=int(out[3]),
                lds=bool(out[4]))


def vi_form_names():
    """The names the single-model value-iteration calls (vi_solve, vi_solve_v, vi_sweeps, vi_backup) record for
    Context.last_kernel_variant() (mp_vi_form_names; host only).  They are not part of kernel_form_names()."""
    return load().mp_vi_form_names().decode().split()


VI_V_PLACEMENT = ("global", "lds", "pieces")


def vi_geometry(mode, S=1, A=1, M=1, Sc=None, cus=256):
    """Host arithmetic of a single-model value-iteration launch (mp_vi_geometry; no device) on a device of ``cus`` compute
    units; the MP_VI_* knobs are read from the environment.  ``mode`` "deterministic": M models of S states and A actions ->
    dict(small_lds, small_fits, small, persist_block, persist_wgs, persist); ``mode`` "stochastic": dense rows of ``Sc`` columns
    -> dict(nb, nbt, waves, fixed_lds, v_default, v, nseg, seg_cols), the V placements as "lds" | "pieces" | "global"."""
    out = np.zeros(14, np.int64)
    code = {"deterministic": MODE_DETERMINISTIC, "stochastic": MODE_STOCHASTIC}[mode]
    _check(load().mp_vi_geometry(code, int(S), int(A), int(M), int(S if Sc is None else Sc), int(cus), _ptr(out)))
    if mode == "deterministic":
        return dict(small_lds=int(out[0]), small_fits=bool(out[1]), small=bool(out[2]), persist_block=int(out[3]),
                    persist_wgs=int(out[4]), persist=bool(out[5]))
    return dict(nb=int(out[6]), nbt=int(out[7]), waves=int(out[8]), fixed_lds=int(out[9]), v_default=VI_V_PLACEMENT[out[10]],
                v=VI_V_PLACEMENT[out[11]], nseg=int(out[12]), seg_cols=int(out[13]))


VI_BATCH_FORMS = ("reg", "cluster", "wg_stream", "wg_lds", "wg_global")


def vi_batch_geometry(N, Sb, A, iterations=1, cus=256):
    """The kernel form ``vi_solve_batch`` chooses for N MDPs of Sb states and A actions on a device of ``cus`` compute units
    (mp_vi_batch_geometry; host only, the function the solve launches from); the MP_VI_BATCH_* knobs are read from the
    environment -> dict(form = one of VI_BATCH_FORMS, name = what Context.last_kernel_variant() reports, at = the compile-time
    |A| or 0, own = states a thread keeps in registers, block, k = workgroups per MDP, grid, lds = dynamic LDS bytes)."""
    out = np.zeros(7, np.int64)
    name = C.c_char_p()
    _check(load().mp_vi_batch_geometry(int(N), int(Sb), int(A), int(iterations), int(cus), _ptr(out), C.byref(name)))
    return dict(form=VI_BATCH_FORMS[out[0]], name=name.value.decode(), at=int(out[1]), own=int(out[2]), block=int(out[3]),
                k=int(out[4]), grid=int(out[5]), lds=int(out[6]))


def vi_exact_plan(n):
    """The tables the bit-exact dense backup sums a row of ``n`` elements by (numpy's pairwise recursion; host only):
    -> (leaves int32 [L,2] {offset, length}, nodes int32 [K,2] {left slot, right slot} by height, hoff int32 [H+1],
    most 8-element steps in a leaf).  Leaf l is slot l, addition k slot L + k; the last slot holds the sum."""
    lib = load()
    counts = np.zeros(4, dtype=np.int32)
    _check(lib.mp_vi_exact_plan(int(n), 0, None, 0, None, 0, None, _ptr(counts)))
    leaves = np.zeros((int(counts[0]), 2), dtype=np.int32)
    nodes = np.zeros((int(counts[1]), 2), dtype=np.int32)
    hoff = np.zeros(int(counts[2]) + 1, dtype=np.int32)
    _check(lib.mp_vi_exact_plan(int(n), len(leaves), _ptr(leaves), len(nodes), _ptr(nodes) if len(nodes) else None,
                                len(hoff) - 1, _ptr(hoff), _ptr(counts)))
    return leaves, nodes, hoff, int(counts[3])


class Context(object):
    """One GPU + stream + workspaces (mp_ctx).  `stream` = raw hipStream_t (int) or None."""

    def __init__(self, device=0, stream=None):
        self._lib = load()
        h = _vp()
        _check(self._lib.mp_ctx_create(int(device), _vp(stream) if stream else None, C.byref(h)))
        self._h = h
        self.device = int(device)

    @classmethod
    def on_torch_stream(cls, device=0):
        """Context enqueuing on a torch side stream of `device` (kept as ``ctx.torch_stream``): run torch work
        under ``with torch.cuda.stream(ctx.torch_stream)`` and torch events / allocations interoperate."""
        import torch
        with torch.cuda.device(device):
            stream = torch.cuda.Stream(device=device)
            ctx = cls(device, stream.cuda_stream)
            ctx.torch_stream = stream
            return ctx

    def close(self):
        if getattr(self, "_h", None):
            for buf in self.__dict__.pop("_pin_cache", {}).values():
                buf.close()
            self._lib.mp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        """Wait for the context's stream; raises NativeError(MP_ERR_ARG) if a device-array plan since the last synchronisation
        had to clamp out-of-range roots (mp_ctx_synchronize)."""
        _check(self._lib.mp_ctx_synchronize(self._h))

    def device_faults(self):
        """Roots clamped by device-array plans on batch models since the last synchronize() (exact once the work was waited for)."""
        n = c_i32()
        _check(self._lib.mp_ctx_device_faults(self._h, C.byref(n)))
        return int(n.value)

    def set_stream(self, stream):
        """Enqueue on another hipStream_t from now on (raw pointer, e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        _check(self._lib.mp_ctx_set_stream(self._h, _vp(stream) if stream else None))

    def stream_ptr(self):
        """The raw hipStream_t this context enqueues on (``torch.cuda.ExternalStream(ptr)`` wraps it)."""
        st = _vp()
        _check(self._lib.mp_ctx_get_stream(self._h, C.byref(st)))
        return st.value or 0

    def device_info(self):
        cu, wave, lds, hbm = c_i32(), c_i32(), c_i64(), c_i64()
        name = C.create_string_buffer(256)
        _check(self._lib.mp_ctx_device_info(self._h, C.byref(cu), C.byref(wave), C.byref(lds), C.byref(hbm), name, 256))
        return dict(n_cu=cu.value, wave_size=wave.value, lds_bytes=lds.value, hbm_bytes=hbm.value,
                    name=name.value.decode())

    def last_kernel_ms(self):
        ms, n = c_f64(), c_i32()
        _check(self._lib.mp_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_kernel_variant(self):
        """Which kernel form the last plan / value-iteration call launched ("uct_ldsr", "opd_wide_sib_small", "saopd_wave_dict", ...:
        every name in kernel_form_names(); after a Sparse Sampling plan one of ss_form_names(), after a single-model
        value-iteration call (vi_solve, vi_solve_v, vi_sweeps, vi_backup) one of vi_form_names() -- the launch that produced the
        returned values -- neither of which that list holds)."""
        return self._lib.mp_last_kernel_variant(self._h).decode()

    def uct_last_action_table(self):
        """Whether the last uct_plan* call launched its form ("uct_ldsr") with the rollout's action table in LDS
        (mp_uct_last_action_table): False with MP_UCT_ACTION_TABLE=0, for any other form, for |A| > 6 and for a model that leaves
        the table no room.  The form's name and the results are the same either way."""
        return bool(self._lib.mp_uct_last_action_table(self._h))

    def vi_graph_captures(self):
        """How many times this context has captured a chain of deterministic value-iteration sweeps into a graph
        (mp_vi_graph_captures): a "vi_det_chain_*_graph" call whose key -- model, pointers, sizes, iterations, gamma, tolerances,
        Q or V form -- is the cached one replays the graph and leaves the count alone."""
        return int(self._lib.mp_vi_graph_captures(self._h))

    # ---- the collective of the C ABI (RCCL resolved at run time): what a consumer without torch.distributed calls ------------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL unique id (rank 0 creates it, the caller distributes it)."""
        uid = np.zeros(128, dtype=np.uint8)
        _check(load().mp_comm_unique_id(_ptr(uid)))
        return uid

    def comm_init(self, rank, world, uid):
        uid = np.ascontiguousarray(uid, dtype=np.uint8).reshape(128)
        _check(self._lib.mp_comm_init(self._h, int(rank), int(world), _ptr(uid)))

    def gather_results(self, packed, gathered, stream=None):
        """ncclAllGather of this rank's packed rows (uint8 device tensor [per, row_bytes]) into ``gathered`` [world * per, row_bytes]."""
        _check(self._lib.mp_gather_results(self._h, _vp(stream) if stream else None, int(packed.shape[0]), int(packed.shape[1]),
                                           _ptr(packed), _ptr(gathered)))

    def comm_destroy(self):
        _check(self._lib.mp_comm_destroy(self._h))

    def selftest_sincos(self, x, variant):
        """(sin, cos) of ``x`` evaluated by the DEVICE's restated libm functions in form ``variant`` (mp_selftest_sincos)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        s, c = np.zeros_like(x), np.zeros_like(x)
        _check(self._lib.mp_selftest_sincos(self._h, int(x.size), _ptr(x), int(variant), _ptr(s), _ptr(c)))
        return s, c

    def selftest_olop_bound(self, what, x, y=None, count=None):
        """What the DEVICE's OLOP code computes, one input per lane (mp_selftest_olop_bound).  ``what``: "kl_upper_bound"
        (x = cumulative rewards, count, y = thresholds) -> (bounds, Newton iterations, decision masks: 1 / 2 the in-loop upper /
        lower clamp, 4 the finite difference, 8 / 16 the final lower / upper clamp); "kl_lower_bound": the same for the lower
        bound (MDP-GapE's mu_lcb); "bernoulli_kl" (p = x, q = y) -> values; "log" -> values."""
        code = {"kl_upper_bound": 0, "bernoulli_kl": 1, "log": 2, "kl_lower_bound": 3}[what]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        n = x.size
        out = np.zeros(n, np.float64)
        if code == 2:
            _check(self._lib.mp_selftest_olop_bound(self._h, code, n, _ptr(x), None, None, _ptr(out), None, None))
            return out
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if y.size != n:
            raise ValueError("selftest_olop_bound: x and y differ in length")
        if code == 1:
            _check(self._lib.mp_selftest_olop_bound(self._h, code, n, _ptr(x), _ptr(y), None, _ptr(out), None, None))
            return out
        count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        if count.size != n:
            raise ValueError("selftest_olop_bound: x and count differ in length")
        its, mask = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(self._lib.mp_selftest_olop_bound(self._h, code, n, _ptr(x), _ptr(y), _ptr(count), _ptr(out), _ptr(its), _ptr(mask)))
        return out, its, mask

    def selftest_lds_atomic_order(self, waves=65536):
        """Violations of "same-address LDS atomics of one wave instruction apply in lane order" (0 on a conforming device)."""
        v = C.c_int64(-1)
        _check(self._lib.mp_selftest_lds_atomic_order(self._h, int(waves), C.byref(v)))
        return int(v.value)

    # ---- host-inclusive fast path: pinned arrays, device-resident generator records -------------------------
    def pinned(self, spec):
        """``{name: (shape, dtype)}`` -> :class:`PinnedArrays`: numpy views of ONE pinned host block (mp_host_alloc).
        Copies from / to them are asynchronous DMA; pass them where host arrays are expected."""
        return PinnedArrays(self, spec)

    def plan_buffers(self, n_roots, max_plan_len, n_actions=None, outputs=("plans", "plan_len", "root_value", "env_steps")):
        """Pinned, reusable host arrays for batched plan() calls of ``n_roots`` roots: the ``root_state`` input and the
        requested ``outputs`` (``uct_plan(..., out=buffers)`` fills exactly those; outputs not listed are not computed
        into host memory at all).  The caller owns them: a later call with the same buffers overwrites the results."""
        n, mpl = int(n_roots), int(max_plan_len)
        shapes = dict(root_state=((n,), np.int32))
        for family in ("uct", "opd"):
            shapes.update(_result_spec(family, n, L=mpl, A=None if n_actions is None else int(n_actions)))
        return PinnedArrays(self, {k: shapes[k] for k in ["root_state"] + list(outputs)})

    # Host-array plans of FEW roots (a single agent's act(): one root) are made through pinned scratch arrays the context
    # keeps: the kernel reads and writes them in place (zero-copy) and the call is one launch + one synchronisation instead of
    # nine pageable copies, each a driver round trip longer than the data (MCTSAgent.act 0.40 -> ms: tools/agent_latency.py).
    SMALL_PLAN_ROOTS = 64

    def _scratch(self, kind, n, spec):
        cache = self.__dict__.setdefault("_pin_cache", {})
        key = (kind, n) + tuple((k,) + tuple(v[0]) for k, v in spec.items())
        buf = cache.get(key)
        if buf is None:
            if len(cache) >= 8:                                  # a handful of shapes per process: evict the oldest
                cache.pop(next(iter(cache))).close()
            buf = cache[key] = PinnedArrays(self, spec)
        return buf

    def _small_plan(self, family, n, mpl, n_actions=None):
        """The scratch arrays of a small ``family`` plan, looked up by the plan's shape alone -> (arrays, their addresses, the
        result arrays among them, those arrays' addresses in the order of the C arguments).  (Building the spec and asking numpy
        for ten ctypes addresses cost a single agent's act() ~10 us of its ~120 -- tools/act_profile.py.)"""
        small = self.__dict__.setdefault("_small_plans", {})
        hit = small.get((family, n, mpl, n_actions))
        if hit is None or hit[0]._ptr is None:          # (evicted from the pinned-array cache: freed)
            spec = {k: ((n,) + tail, dtype) for k, dtype, tail in SCRATCH_INPUTS[family]}
            spec.update(_result_spec(family, n, L=mpl, A=n_actions))
            scratch = self._scratch(family, n, spec)
            if len(small) >= 8:
                small.clear()
            out = {k: scratch[k] for k, _, _, _ in RESULTS[family]}
            hit = small[(family, n, mpl, n_actions)] = (scratch, {k: v.ctypes.data for k, v in scratch.items()}, out,
                                                         [v.ctypes.data for v in out.values()])
        return hit

    def device_rng(self, states_or_n):
        """Generator records resident on the device (mp_rng): an int n (uninitialised) or a uint64 [n, 6] array."""
        if isinstance(states_or_n, (int, np.integer)):
            return DeviceRng(self, int(states_or_n))
        st = np.ascontiguousarray(states_or_n, dtype=np.uint64).reshape(-1, 6)
        rng = DeviceRng(self, st.shape[0])
        rng.set(st)
        return rng

    # ---- batched evaluation on the device ------------------------------------------------------------------------
    def env_step_device(self, model, state, steps, alive, plans, max_steps, gpow, returns, discounted, actions_log, n_alive):
        """One lock-step env.step of every live episode (mp_env_step): all arguments are device tensors; only enqueues."""
        n = int(state.shape[0])
        _check(self._lib.mp_env_step(self._h, model._h, n, _ptr(state), _ptr(steps), _ptr(alive), _ptr(plans),
                                     int(plans.shape[1]), int(max_steps), _ptr(gpow), _ptr(returns), _ptr(discounted),
                                     _ptr(actions_log), 0 if actions_log is None else int(actions_log.shape[1]),
                                     _ptr(n_alive), MP_MEM_DEVICE))

    def env_step_stochastic_device(self, model, state, steps, alive, plans, max_steps, gpow, returns, discounted, actions_log,
                                   n_alive, env_rng):
        """mp_env_step_stochastic: env_step_device for stochastic / sparse models; env_rng int64 [n, 6] device records of the
        episodes' own env generators, advanced in place."""
        n = int(state.shape[0])
        _check(self._lib.mp_env_step_stochastic(self._h, model._h, n, _ptr(state), _ptr(steps), _ptr(alive), _ptr(plans),
                                                int(plans.shape[1]), int(max_steps), _ptr(gpow), _ptr(returns), _ptr(discounted),
                                                _ptr(actions_log), 0 if actions_log is None else int(actions_log.shape[1]),
                                                _ptr(n_alive), _ptr(env_rng), MP_MEM_DEVICE))

    def uct_plan_stochastic_device(self, model, n_roots, root_state, episodes, horizon, gamma, temperature, prior_p, rollout_p,
                                   rng_state, env_rng_state, max_plan_len, closed_loop=False, plans=None, plan_len=None,
                                   root_value=None, env_steps=None, root_steps=None, policy=None):
        """mp_uct_plan_stochastic / _policy on device tensors; only enqueues."""
        pp, rp = (None, None) if policy is not None else _priors(prior_p, rollout_p)
        self._uct_stoch_call(MP_MEM_DEVICE, model, int(n_roots), _ptr(root_state), _ptr(root_steps), episodes, horizon, gamma,
                             temperature, _ptr(pp), _ptr(rp), closed_loop, _ptr(rng_state), _ptr(env_rng_state),
                             int(max_plan_len), _ptrs(plans, plan_len, root_value, None, None, env_steps), policy)

    def greedy_actions_device(self, q, state, plans):
        """plans[:, 0] = argmax_a q[state, a] (first maximum), device tensors."""
        _check(self._lib.mp_greedy_actions(self._h, int(state.shape[0]), int(q.shape[0]), int(q.shape[1]), _ptr(q),
                                           _ptr(state), _ptr(plans), int(plans.shape[1]), MP_MEM_DEVICE))

    # ---- result exchange of the sharded path (mp_pack_rows / mp_unpack_rows): device tensors, only enqueues ------------
    @staticmethod
    def _row_args(arrays):
        ptrs = (_vp * len(arrays))(*[_ptr(a) for a in arrays])
        widths = (c_i32 * len(arrays))(*[int(a.element_size()) * int(np.prod(tuple(a.shape[1:]), dtype=np.int64))
                                         for a in arrays])
        return ptrs, widths

    def pack_rows(self, arrays, n_local, packed, stream=None):
        """Per-root device arrays [n_local, ...] -> rows of ``packed`` (uint8 [per, row_bytes]); padding rows zeroed."""
        ptrs, widths = self._row_args(arrays)
        _check(self._lib.mp_pack_rows(self._h, _vp(stream) if stream else None, int(n_local), int(packed.shape[0]),
                                      len(arrays), ptrs, widths, _ptr(packed)))

    def unpack_rows(self, gathered, n_total, world, arrays, stream=None):
        """``gathered`` (uint8 [world * per, row_bytes], rank-major) -> the full per-root arrays [n_total, ...]."""
        ptrs, widths = self._row_args(arrays)
        _check(self._lib.mp_unpack_rows(self._h, _vp(stream) if stream else None, int(n_total), int(world),
                                        int(gathered.shape[0]) // int(world), len(arrays), _ptr(gathered), widths, ptrs))

    # ---- models ------------------------------------------------------------------------------
    def load_table(self, transition, reward, terminal=None, done_rule="source", max_steps=0, available=None):
        """Deterministic tables: transition int [S,A] or [M,S,A], reward like it, terminal [S].
        available: bool [S,A], the actions state.get_available_actions() lists per state (None = all)."""
        t, r = _int_tables(transition, reward, (2, 3), "transition and reward must both be [S, A] (or [M, S, A])")
        m = 1 if t.ndim == 2 else t.shape[0]
        s, a = t.shape[-2:]
        term = _flags(terminal, s)
        h = _vp()
        _check(self._lib.mp_model_load_table(self._h, m, s, a, _ptr(t), _ptr(r), _ptr(term),
                                             int(done_rule == "next"), int(max_steps or 0), C.byref(h)))
        model = Model(self, h, MODE_DETERMINISTIC, m, s, a, 0)
        if available is not None:
            av = _flags(available, s, a)
            _check(self._lib.mp_model_set_available(h, _ptr(av)))
            model.available = av.astype(bool)
        return model

    def load_table_batch(self, transition, reward, terminal=None, done_rule="source", max_steps=0):
        """A batch of N independent deterministic MDPs of one shape (mp_model_load_table_batch): transition int [N,S,A]
        (states LOCAL to each MDP), reward [N,S,A], terminal [N,S] or None -> one :class:`Model` over the N * S GLOBAL
        states ``b * S + s`` (``model.n_models``, ``model.S_each``); every deterministic-table entry point takes it, the
        planners with ``model_index=`` (one MDP per root) or with global root states."""
        t, r = _int_tables(transition, reward, (3,), "transition and reward must both be [N, S, A]")
        n, s, a = t.shape
        term = _flags(terminal, n, s)
        h = _vp()
        _check(self._lib.mp_model_load_table_batch(self._h, n, s, a, _ptr(t), _ptr(r), _ptr(term), int(done_rule == "next"),
                                                   int(max_steps or 0), C.byref(h)))
        model = Model(self, h, MODE_DETERMINISTIC, 1, n * s, a, 0)
        model.n_models, model.S_each = n, s
        return model

    def vi_solve_batch(self, model, gamma, iterations, rtol=1e-5, atol=1e-8):
        """N value-iteration agents in one launch (mp_vi_solve_batch) -> (Q float64 [N,S,A], sweeps int32 [N]): each MDP of
        the batch model runs to its own allclose exit, bit-equal to N :meth:`vi_solve` calls on the N tables."""
        q = np.zeros((model.n_models, model.S_each, model.A), dtype=np.float64)
        sweeps = np.zeros(model.n_models, dtype=np.int32)
        _check(self._lib.mp_vi_solve_batch(self._h, model._h, float(gamma), int(iterations), float(rtol), float(atol),
                                           _ptr(q), _ptr(sweeps), MP_MEM_HOST))
        return q, sweeps

    def vi_solve_batch_device(self, model, gamma, iterations, q_out, sweeps_out, rtol=1e-5, atol=1e-8):
        """Asynchronous form on device tensors: q_out float64 [N*S, A] (what ``greedy_actions_device`` takes with global
        states), sweeps_out int32 [N]; only enqueues."""
        _check(self._lib.mp_vi_solve_batch(self._h, model._h, float(gamma), int(iterations), float(rtol), float(atol),
                                           _ptr(q_out), _ptr(sweeps_out), MP_MEM_DEVICE))

    def load_joint(self, transitions, rewards, terminals=None, done_rule="source", available=None):
        """A joint environment of M models (agents/robust/robust.py:9-26): transitions int [M,S,A], rewards [M,S,A],
        terminals [M,S] (each model's own flags) or None.  available: bool [M,S,A], what each model's env lists in
        get_available_actions() (the joint env lists the union over its models' states, robust.py:22-25); None = all."""
        t, r = _int_tables(transitions, rewards, (3,), "transitions and rewards must both be [M, S, A]")
        m, s, a = t.shape
        term = _flags(terminals, m, s)
        h = _vp()
        _check(self._lib.mp_model_load_joint(self._h, m, s, a, _ptr(t), _ptr(r), _ptr(term), int(done_rule == "next"),
                                             C.byref(h)))
        model = Model(self, h, MODE_DETERMINISTIC, m, s, a, 0)
        if available is not None:
            av = _flags(available, m, s, a)
            _check(self._lib.mp_model_set_available_joint(h, _ptr(av)))
            model.available = av.astype(bool)
        return model

    def load_joint_batch(self, transitions, rewards, terminals=None, done_rule="source", available=None):
        """N sets of M models of one (S, A) shape (mp_model_load_joint_batch): what N robust agents that build their models
        again before every plan hold (agents/robust/robust.py:68-71).  transitions int [N,M,S,A] (next states LOCAL to each
        table), rewards [N,M,S,A], terminals [N,M,S] or None, available bool [N,M,S,A] or None -> a :class:`JointBatchModel`
        (``n_models`` = N sets, ``M``, ``S_each``); :meth:`ropd_plan` takes it with ``model_index=``."""
        t, r = _int_tables(transitions, rewards, (4,), "transitions and rewards must both be [N, M, S, A]")
        n, m, s, a = t.shape
        term = _flags(terminals, n, m, s)
        h = _vp()
        _check(self._lib.mp_model_load_joint_batch(self._h, n, m, s, a, _ptr(t), _ptr(r), _ptr(term), int(done_rule == "next"),
                                                   C.byref(h)))
        model = JointBatchModel(self, h, MODE_DETERMINISTIC, m, n * s, a, 0)
        model.n_models, model.S_each = n, s
        if available is not None:
            model.set_available(available)
        return model

    @staticmethod
    def _dense_arrays(transition, reward, terminal, square):
        """What load_dense and load_dense_rows hand the library -> (transition, reward, terminal flags, transition's shape,
        MP_MEM_*, the arrays to keep alive): torch tensors are borrowed as they are, anything else is copied to float64 /
        uint8 host arrays (``square``: one terminal flag per column)."""
        if hasattr(transition, "data_ptr"):
            return transition, reward, terminal, tuple(transition.shape), MP_MEM_DEVICE, (transition, reward, terminal)
        t = np.ascontiguousarray(transition, dtype=np.float64)
        term = _flags(terminal, t.shape[-1]) if square else _flags(terminal)
        return t, np.ascontiguousarray(reward, dtype=np.float64), term, t.shape, MP_MEM_HOST, None

    def load_dense(self, transition, reward, terminal=None):
        """Dense model: transition float [S,A,S] or [M,S,A,S] (numpy -> copied; torch cuda tensor -> borrowed)."""
        t, r, term, shape, mem, keep = self._dense_arrays(transition, reward, terminal, True)
        if mem == MP_MEM_DEVICE and not (t.is_contiguous() and r.is_contiguous()):
            raise ValueError("device arrays must be contiguous")
        if len(shape) not in (3, 4) or shape[-1] != shape[-3]:
            raise ValueError("transition must be [S, A, S] (or [M, S, A, S])")
        m = 1 if len(shape) == 3 else shape[0]
        s, a = shape[-3], shape[-2]
        h = _vp()
        _check(self._lib.mp_model_load_dense(self._h, m, s, a, _ptr(t), _ptr(r), _ptr(term), mem, C.byref(h)))
        mod = Model(self, h, MODE_STOCHASTIC, m, s, a, 0)
        mod._keep = keep
        return mod

    def load_dense_rows(self, transition, reward, terminal=None):
        """Row block of a dense model: transition [S_rows,A,S] or [M,S_rows,A,S] (numpy copied / torch borrowed),
        reward [..,S_rows,A], terminal [S_rows] flags of the owned rows."""
        t, r, term, shape, mem, keep = self._dense_arrays(transition, reward, terminal, False)
        m = 1 if len(shape) == 3 else shape[0]
        rows, a, cols = shape[-3], shape[-2], shape[-1]
        h = _vp()
        _check(self._lib.mp_model_load_dense_rows(self._h, m, rows, a, cols, _ptr(t), _ptr(r), _ptr(term), mem, C.byref(h)))
        mod = Model(self, h, MODE_STOCHASTIC, m, rows, a, 0)
        mod.S_cols = cols
        mod._keep = keep
        return mod

    def vi_backup(self, model, gamma, v, q_out=None, robust=False):
        """One Bellman backup of a dense / row-block model. numpy in -> numpy out; torch tensors -> enqueued only."""
        if hasattr(v, "data_ptr"):
            _check(self._lib.mp_vi_backup(self._h, model._h, float(gamma), int(bool(robust)), _ptr(v), _ptr(q_out),
                                          MP_MEM_DEVICE))
            return q_out
        v = np.ascontiguousarray(v, dtype=np.float64)
        q = np.zeros((model.S, model.A), dtype=np.float64) if q_out is None else q_out
        _check(self._lib.mp_vi_backup(self._h, model._h, float(gamma), int(bool(robust)), _ptr(v), _ptr(q), MP_MEM_HOST))
        return q

    def load_sparse(self, transition, next_states, reward, terminal=None):
        t = np.ascontiguousarray(transition, dtype=np.float64)
        n = np.ascontiguousarray(next_states, dtype=np.int64)
        r = np.ascontiguousarray(reward, dtype=np.float64)
        _same_shape(t, n, (3,), "next and transition must both be [S, A, B]")
        s, a, b = t.shape
        term = _flags(terminal, s)
        h = _vp()
        _check(self._lib.mp_model_load_sparse(self._h, s, a, b, _ptr(t), _ptr(n), _ptr(r), _ptr(term), C.byref(h)))
        return Model(self, h, MODE_SPARSE, 1, s, a, b)

    def load_cartpole(self, params):
        """Closed-form CartPole model from ``CartPoleEnv.cartpole_params()`` (dict)."""
        cp = CartPoleParams(**{k: params[k] for k, _ in CartPoleParams._fields_})
        if libm_sincos_variant() not in (1, 2) and not os.environ.get("MP_CARTPOLE_SINCOS"):
            # neither restated glibc form reproduces THIS host's libm sin / cos: the device falls back to its own math library
            # and plans may differ from the reference's in the last bits of a pole angle -- say so, loudly, once per load
            import warnings
            warnings.warn("CartPole model: no restated form of sin / cos matches this host's libm (mp_libm_sincos_variant() == 0): "
                          "the device uses its own sincos and bit-exact parity with the CPU reference is NOT guaranteed",
                          RuntimeWarning, stacklevel=2)
        h = _vp()
        _check(self._lib.mp_model_load_cartpole(self._h, C.addressof(cp), C.byref(h)))
        return Model(self, h, MODE_CARTPOLE, 1, 0, 2, 0)

    # ---- value iteration ---------------------------------------------------------------------
    def vi_solve(self, model, gamma, iterations, robust=False, rtol=1e-5, atol=1e-8):
        """-> (Q [S,A] float64, sweeps run).  value_iteration.py:42-45,65-73 / robust_value_iteration.py:39-58."""
        q = np.zeros((model.S, model.A), dtype=np.float64)
        sweeps = np.zeros(1, dtype=np.int32)
        _check(self._lib.mp_vi_solve(self._h, model._h, float(gamma), int(iterations), float(rtol), float(atol),
                                     int(bool(robust)), _ptr(q), _ptr(sweeps), MP_MEM_HOST))
        if sweeps[0] < 0:       # (the host-mode call re-solves by itself when the persistent kernel gives up: not reached)
            raise NativeError(MP_ERR_HIP, "value iteration failed on the device (sweeps = {})".format(int(sweeps[0])))
        return q, int(sweeps[0])

    def vi_solve_v(self, model, gamma, iterations, rtol=1e-5, atol=1e-8, robust=False):
        """get_state_value: value_iteration.py:37-40, or robust_value_iteration.py:32-37 with robust=True."""
        v = np.zeros(model.S, dtype=np.float64)
        fn = self._lib.mp_vi_solve_v_robust if robust else self._lib.mp_vi_solve_v
        _check(fn(self._h, model._h, float(gamma), int(iterations), float(rtol), float(atol), _ptr(v), MP_MEM_HOST))
        return v

    def vi_solve_device(self, model, gamma, iterations, q_out, sweeps_out, robust=False, rtol=1e-5, atol=1e-8):
        """Asynchronous solve into device tensors (q_out float64 [S,A], sweeps_out int32 [1]).  Nothing is read back:
        ``sweeps_out[0] == -1`` (with NaN in ``q_out``) reports that the single-launch solver of small deterministic
        models could not keep its grid resident (GPU shared with other work) -- check it where the result is consumed
        (:func:`check_device_sweeps`), or use :meth:`vi_solve`, which re-solves by itself."""
        _check(self._lib.mp_vi_solve(self._h, model._h, float(gamma), int(iterations), float(rtol), float(atol),
                                     int(bool(robust)), _ptr(q_out), _ptr(sweeps_out), MP_MEM_DEVICE))

    def vi_sweeps(self, model, gamma, sweeps, robust=False):
        _check(self._lib.mp_vi_sweeps(self._h, model._h, float(gamma), int(sweeps), int(bool(robust))))

    def vi_dense_mode(self, mode):
        """How dense models are contracted with V: ``"mfma"`` (f64 matrix cores, tolerance parity) or ``"exact"``
        (numpy's own order of roundings and additions: Q, V and sweep counts bit-equal to the reference's)."""
        _check(self._lib.mp_vi_dense_mode(self._h, {"mfma": 0, "exact": 1}[mode]))

    # ---- tree search -------------------------------------------------------------------------
    def load_policy(self, model, prior, rollout, listed=None, rollout_slots=None):
        """Per-state prior / rollout policies [S, A] of a table model (mcts_with_prior.py:47-62) -> Policy.
        listed: bool [S, A], the actions the prior policy lists per state (restricted action sets, mcts.py:59-97):
        only those get a child at expansion; None = all.  rollout_slots: uint8 [S, A], the order in which the rollout
        policy lists the columns of each state when it is not the column order (mp_policy_load_ordered).
        On a batch model the tables may also be [S_each, A]: rows over the LOCAL states of one MDP that serve every MDP of the
        batch (mp_policy_load_rows)."""
        pr = np.ascontiguousarray(prior, dtype=np.float64)
        ro = pr if rollout is prior else np.ascontiguousarray(rollout, dtype=np.float64)
        rows = model.S
        if getattr(model, "n_models", 1) > 1 and pr.shape == (model.S_each, model.A):
            rows = model.S_each
        if pr.shape != (rows, model.A) or ro.shape != (rows, model.A):
            raise ValueError("prior / rollout must be [S, A] = [{}, {}]".format(model.S, model.A))
        h = _vp()
        li, sl = _flags(listed, rows, model.A), _flags(rollout_slots, rows, model.A)
        _check(self._lib.mp_policy_load_rows(self._h, model._h, _ptr(pr), _ptr(ro), _ptr(li), _ptr(sl), int(rows), C.byref(h)))
        return Policy(self, h, model)

    def uct_plan(self, model, root_state, episodes, horizon, gamma, temperature, prior_p, rollout_p, rng_state,
                 root_steps=None, max_plan_len=None, policy=None, out=None, model_index=None):
        """MCTS.plan for a batch of roots (host arrays). rng_state uint64 [n,6] is advanced in place (or a
        :class:`DeviceRng`, advanced on the device).  policy (load_policy): per-state policies instead of prior_p /
        rollout_p.  out (plan_buffers): caller-owned pinned result arrays; only the outputs they hold are produced."""
        if model.mode == MODE_CARTPOLE:      # roots are (x, x_dot, theta, theta_dot) rows
            rs = np.ascontiguousarray(root_state, dtype=np.float64).reshape(-1, 4)
        else:
            rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        n = rs.shape[0]
        st = None if root_steps is None else np.ascontiguousarray(root_steps, dtype=np.int32).reshape(n)
        mem, rng_ptr = self._rng_arg(rng_state, n)
        mi = None
        if model_index is not None:             # batch model: root i plans on MDP model_index[i] from its LOCAL state
            mi = np.ascontiguousarray(model_index, dtype=np.int32).reshape(n)
            if policy is not None:              # (policies are tables over the global states: no second index needed)
                rs = (mi * np.int32(model.S_each) + rs).astype(np.int32)
                mi = None
        scratch = None
        if out is not None:                     # caller-owned (pinned) buffers: only the outputs they hold are produced
            mpl = out["plans"].shape[1] if "plans" in out else 0
            for k in out:
                if k != "root_state" and out[k].shape[0] != n:
                    raise ValueError("output buffer '{}' holds {} roots, the batch has {}".format(k, out[k].shape[0], n))
        elif (n <= self.SMALL_PLAN_ROOTS and mem == MP_MEM_HOST and mi is None and model.mode != MODE_CARTPOLE
              and not os.environ.get("MP_NO_PINNED_SCRATCH")):
            mpl = int(horizon if max_plan_len is None else max_plan_len)
            scratch, sp, out, o = self._small_plan("uct", n, mpl, int(model.A))
            scratch["root_state"][:] = rs
            scratch["rng"][:] = rng_state.reshape(n, 6)
            scratch["plans"][:] = -1
            if st is not None:
                scratch["root_steps"][:] = st
            if policy is None:                  # (a single agent's act(): the scratch arrays' addresses are the cached ones)
                pp, rp = _priors(prior_p, rollout_p, model.A)
                self._uct_call(mem, model, n, sp["root_state"], None if st is None else sp["root_steps"], episodes, horizon, gamma,
                               temperature, pp.ctypes.data, rp.ctypes.data, sp["rng"], mpl, o)
                return self._from_scratch(scratch, out, rng_state)
            rs, rng_ptr = scratch["root_state"], sp["rng"]
            if st is not None:
                st = scratch["root_steps"]
        else:
            mpl = int(horizon if max_plan_len is None else max_plan_len)
            out = _results("uct", n, L=mpl, A=model.A)
        o = _result_ptrs("uct", out)
        pp, rp = (None, None) if policy is not None else _priors(prior_p, rollout_p, model.A)
        self._uct_call(mem, model, n, _ptr(rs), _ptr(st), episodes, horizon, gamma, temperature, _ptr(pp), _ptr(rp), rng_ptr, mpl,
                       o, policy, _ptr(mi))
        return self._from_scratch(scratch, out, rng_state)

    def _uct_call(self, mem, model, n, rs, st, episodes, horizon, gamma, temperature, pp, rp, rng, mpl, o, policy=None, mi=None):
        """The one call of mp_uct_plan and of its _policy / _models entry points: every array is an address (``o``: those of
        the six results), ``mem`` says where they live."""
        run = (int(episodes), int(horizon), float(gamma), float(temperature))
        if policy is not None:
            _check(self._lib.mp_uct_plan_policy(self._h, model._h, policy._h, n, rs, st, *run, rng, mpl, *o, mem))
        elif mi is not None:
            _check(self._lib.mp_uct_plan_models(self._h, model._h, n, mi, rs, st, *run, pp, rp, rng, mpl, *o, mem))
        else:
            _check(self._lib.mp_uct_plan(self._h, model._h, n, rs, st, *run, pp, rp, rng, mpl, *o, mem))

    @staticmethod
    def _from_scratch(scratch, out, rng_state):
        """Results of a small plan leave the context's pinned scratch arrays as the caller's own copies (the generator records
        go back into the caller's array, advanced)."""
        if scratch is None:
            return out
        rng_state.reshape(-1, 6)[:] = scratch["rng"]
        return {k: v.copy() for k, v in out.items()}

    @staticmethod
    def _rng_arg(rng_state, n):
        """(mem flags, pointer) for the generator records of a host-array call: a uint64 [n, 6] numpy array (copied in
        and out) or a :class:`DeviceRng` (resident: MP_MEM_RNG_DEVICE)."""
        if isinstance(rng_state, DeviceRng):
            if rng_state.n < n:
                raise ValueError("the device generator holds {} records, the batch has {} roots".format(rng_state.n, n))
            return MP_MEM_HOST | MP_MEM_RNG_DEVICE, rng_state.ptr(0)
        _check_rng(rng_state, n, or_what=" or a DeviceRng")
        return MP_MEM_HOST, rng_state.ctypes.data

    def uct_plan_device(self, model, n_roots, root_state, episodes, horizon, gamma, temperature, prior_p, rollout_p,
                        rng_state, max_plan_len, plans=None, plan_len=None, root_value=None, root_child_count=None,
                        root_child_value=None, env_steps=None, root_steps=None, policy=None, model_index=None):
        """Same, on device tensors (torch); only enqueues on the ctx stream.  model_index (int32 device tensor): batch
        model, one MDP per root, root_state LOCAL."""
        if model_index is not None and policy is not None:
            raise ValueError("per-state policies on a batch model are indexed by global state: pass global root states")
        pp, rp = (None, None) if policy is not None else _priors(prior_p, rollout_p)
        self._uct_call(MP_MEM_DEVICE, model, int(n_roots), _ptr(root_state), _ptr(root_steps), episodes, horizon, gamma,
                       temperature, _ptr(pp), _ptr(rp), _ptr(rng_state), int(max_plan_len),
                       _ptrs(plans, plan_len, root_value, root_child_count, root_child_value, env_steps), policy, _ptr(model_index))

    def uct_plan_stochastic(self, model, root_state, episodes, horizon, gamma, temperature, prior_p, rollout_p, rng_state,
                            env_rng_state=None, closed_loop=False, root_steps=None, max_plan_len=None, policy=None, visits=None):
        """MCTS.plan on a stochastic (dense / sparse) finite-MDP model, open or closed loop (mp_uct_plan_stochastic).
        env_rng_state uint64 [n,6]: the env generator's record per root at plan time (every episode's clone starts from
        it; not advanced).  closed_loop: plans alternate action, observation key (next state index), action, ..."""
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        n = rs.shape[0]
        st = None if root_steps is None else np.ascontiguousarray(root_steps, dtype=np.int32).reshape(n)
        mem, rng_ptr = self._rng_arg(rng_state, n)
        erng = None if env_rng_state is None else np.ascontiguousarray(env_rng_state, dtype=np.uint64).reshape(n, 6)
        mpl = int((2 if closed_loop else 1) * horizon if max_plan_len is None else max_plan_len)
        out = _results("uct", n, L=mpl, A=model.A)
        if visits is not None:          # int32 [n, S]: how often the plan's env steps land in each state (mp_uct_record_visits)
            if visits.dtype != np.int32 or visits.shape != (n, model.S) or not visits.flags.c_contiguous:
                raise ValueError("visits must be a C-contiguous int32 [n_roots, S] array")
            _check(self._lib.mp_uct_record_visits(self._h, _ptr(visits)))
        # (policy: per-state policies, load_policy on this stochastic model)
        pp, rp = (None, None) if policy is not None else _priors(prior_p, rollout_p, model.A)
        self._uct_stoch_call(mem, model, n, _ptr(rs), _ptr(st), episodes, horizon, gamma, temperature, _ptr(pp), _ptr(rp),
                             closed_loop, rng_ptr, _ptr(erng), mpl, _result_ptrs("uct", out), policy)
        return out

    def _uct_stoch_call(self, mem, model, n, rs, st, episodes, horizon, gamma, temperature, pp, rp, closed_loop, rng, erng, mpl, o,
                        policy=None):
        """The one call of mp_uct_plan_stochastic and of its _policy entry point, on addresses as in :meth:`_uct_call`."""
        run = (int(episodes), int(horizon), float(gamma), float(temperature))
        tail = (int(bool(closed_loop)), rng, erng, mpl) + tuple(o) + (mem,)
        if policy is not None:
            _check(self._lib.mp_uct_plan_stochastic_policy(self._h, model._h, policy._h, n, rs, st, *(run + tail)))
        else:
            _check(self._lib.mp_uct_plan_stochastic(self._h, model._h, n, rs, st, *(run + (pp, rp) + tail)))

    UCT_STOCH_TREE = (("parent", np.int32, ()), ("action", np.int32, ()), ("is_obs", np.uint8, ()), ("count", np.int64, ()),
                      ("value", np.float64, ()))

    def uct_stoch_tree(self, root):
        """Tree of `root` after the last uct_plan_stochastic, creation order: parent, action (= key: action id or observed
        state), is_obs, count, value."""
        c = c_i32()
        _check(self._lib.mp_uct_stoch_tree_capacity(self._h, C.byref(c)))
        t = _export_tree(self._lib.mp_uct_stoch_tree_export, (self._h, int(root)), c.value, self.UCT_STOCH_TREE)
        prior = np.zeros(c.value, np.float64)       # stored child priors (per-state policies; zeros otherwise)
        _check(self._lib.mp_uct_stoch_tree_priors(self._h, c.value, _ptr(prior)))
        t["prior"] = prior[:len(t["parent"])].copy()
        return t

    def uct_step_tree(self, actions):
        """step_strategy 'subtree': keep, for the next uct_plan, the subtree under each root's child actions[i] (a host
        array, or a contiguous int32 device tensor: only enqueues then)."""
        if hasattr(actions, "data_ptr"):
            _check(self._lib.mp_uct_step_tree(self._h, int(actions.shape[0]), _ptr(actions), MP_MEM_DEVICE))
            return
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
        _check(self._lib.mp_uct_step_tree(self._h, a.shape[0], _ptr(a), MP_MEM_HOST))

    def uct_step_tree_select(self, source_root, actions):
        """The same for a batch that shrinks or is re-ordered: the next plan has len(actions) roots, and root j continues the
        subtree under child actions[j] of the LAST plan's root source_root[j] (mp_uct_step_tree_select; host arrays, or
        contiguous int32 device tensors: only enqueues then)."""
        if hasattr(actions, "data_ptr") or hasattr(source_root, "data_ptr"):
            for t in (source_root, actions):    # (an int64 tensor would be read as pairs of int32 values)
                if not (hasattr(t, "data_ptr") and str(t.dtype) == "torch.int32" and t.dim() == 1 and t.is_contiguous() and t.is_cuda):
                    raise ValueError("source_root and actions must both be contiguous one-dimensional int32 device tensors")
            if actions.shape[0] != source_root.shape[0]:
                raise ValueError("source_root and actions must have one entry per new root")
            _check(self._lib.mp_uct_step_tree_select(self._h, int(actions.shape[0]), _ptr(source_root), _ptr(actions), MP_MEM_DEVICE))
            return
        s = np.ascontiguousarray(source_root, dtype=np.int32).reshape(-1)
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
        if s.shape != a.shape:
            raise ValueError("source_root and actions must have one entry per new root")
        _check(self._lib.mp_uct_step_tree_select(self._h, a.shape[0], _ptr(s), _ptr(a), MP_MEM_HOST))

    def uct_reset_tree(self):
        _check(self._lib.mp_uct_reset_tree(self._h))

    UCT_TREE = (("parent", np.int32, ()), ("action", np.int32, ()), ("count", np.int64, ()), ("value", np.float64, ()),
                ("first_child", np.int32, ()), ("n_children", np.int32, ()))

    def uct_tree(self, root, cap=None):
        if cap is None:
            c = c_i32()
            _check(self._lib.mp_uct_tree_capacity(self._h, C.byref(c)))
            cap = c.value
        return _export_tree(self._lib.mp_uct_tree_export, (self._h, int(root)), cap, self.UCT_TREE)

    def uct_path_count(self, root, actions):
        """Visit count of the node the action sequence reaches in the last plan's tree of `root` (-1: it leaves the tree)."""
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
        c = C.c_int64()
        _check(self._lib.mp_uct_path_count(self._h, int(root), _ptr(a) if a.size else None, int(a.size), C.byref(c)))
        return int(c.value)

    def opd_plan(self, model, root_state, budget, gamma, terminal_reward, rng_state, max_plan_len=64, model_index=None):
        """OptimisticDeterministicPlanner.plan for a batch of roots (host arrays).  model_index: batch model, root i plans
        on MDP model_index[i] from its LOCAL state."""
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        return self._opd_plan(False, model, rs, budget, gamma, terminal_reward, rng_state, max_plan_len, model_index)

    def _opd_plan(self, robust, model, rs, budget, gamma, terminal_reward, rng_state, max_plan_len, model_index):
        """opd_plan and ropd_plan behind their root states ``rs`` ([n] / [n, M]); the few roots of a single-model OPD plan go
        through the context's pinned scratch arrays."""
        n = rs.shape[0]
        _check_rng(rng_state, n)
        mpl = int(max_plan_len)
        mi = None if model_index is None else np.ascontiguousarray(model_index, dtype=np.int32).reshape(n)
        scratch, rng = None, rng_state
        if not robust and n <= self.SMALL_PLAN_ROOTS and mi is None and not os.environ.get("MP_NO_PINNED_SCRATCH"):
            scratch, sp, out, o = self._small_plan("opd", n, mpl)
            scratch["root_state"][:] = rs
            scratch["rng"][:] = rng_state.reshape(n, 6)
            scratch["plans"][:] = -1
            rs, rng = scratch["root_state"], scratch["rng"]
        else:
            out = _results("opd", n, L=mpl)
            o = _result_ptrs("opd", out)
        self._opd_call(robust, MP_MEM_HOST, model, n, _ptr(mi), _ptr(rs), budget, gamma, terminal_reward, _ptr(rng), mpl, o)
        return self._from_scratch(scratch, out, rng_state)

    def _opd_call(self, robust, mem, model, n, mi, rs, budget, gamma, terminal_reward, rng, mpl, o):
        """The one call of mp_opd_plan / mp_ropd_plan and of their _models entry points (``mi``: one model (set) per root),
        on addresses."""
        if mi is None:
            fn, roots = self._lib.mp_ropd_plan if robust else self._lib.mp_opd_plan, (n, rs)
        else:
            fn, roots = self._lib.mp_ropd_plan_models if robust else self._lib.mp_opd_plan_models, (n, mi, rs)
        _check(fn(self._h, model._h, *roots, int(budget), float(gamma), float(terminal_reward), rng, mpl, *o, mem))

    def opd_plan_device(self, model, n_roots, root_state, budget, gamma, terminal_reward, rng_state, max_plan_len,
                        plans=None, plan_len=None, root_lower=None, root_upper=None, env_steps=None, status=None, model_index=None):
        self._opd_call(False, MP_MEM_DEVICE, model, int(n_roots), _ptr(model_index), _ptr(root_state), budget, gamma,
                       terminal_reward, _ptr(rng_state), int(max_plan_len),
                       _ptrs(plans, plan_len, root_lower, root_upper, env_steps, status))

    def ropd_plan(self, model, root_state, budget, gamma, terminal_reward, rng_state, max_plan_len=64, model_index=None):
        """DiscreteRobustPlanner.plan for a batch of roots of a joint model; root_state int [n] (every model starts in
        the same state) or [n, M].  model_index int [n]: a joint batch model, root i plans on set model_index[i] from its
        LOCAL joint state (mp_ropd_plan_models)."""
        rs = np.asarray(root_state, dtype=np.int32)
        if rs.ndim == 1:
            rs = np.repeat(rs[:, None], model.M, axis=1)
        rs = np.ascontiguousarray(rs.reshape(-1, model.M))
        return self._opd_plan(True, model, rs, budget, gamma, terminal_reward, rng_state, max_plan_len, model_index)

    def ropd_plan_device(self, model, n_roots, root_state, budget, gamma, terminal_reward, rng_state, max_plan_len,
                         plans=None, plan_len=None, root_lower=None, root_upper=None, env_steps=None, status=None, model_index=None):
        self._opd_call(True, MP_MEM_DEVICE, model, int(n_roots), _ptr(model_index), _ptr(root_state), budget, gamma,
                       terminal_reward, _ptr(rng_state), int(max_plan_len),
                       _ptrs(plans, plan_len, root_lower, root_upper, env_steps, status))

    @staticmethod
    def _opd_tree_fields(*per_model):
        """The node arrays of an OPD tree; robust OPD holds state, reward, bounds and done flag once per model."""
        return (("parent", np.int32, ()), ("action", np.int32, ()), ("state", np.int32, per_model), ("depth", np.int32, ()),
                ("reward", np.float64, per_model), ("lower", np.float64, per_model), ("upper", np.float64, per_model),
                ("done", np.uint8, per_model), ("count", np.int64, ()), ("first_child", np.int32, ()), ("n_children", np.int32, ()))

    def opd_tree(self, root, cap):
        return _export_tree(self._lib.mp_opd_tree_export, (self._h, int(root)), cap, self._opd_tree_fields())

    def ropd_tree(self, root, cap, n_models):
        return _export_tree(self._lib.mp_ropd_tree_export, (self._h, int(root)), cap, self._opd_tree_fields(int(n_models)))

    def _each_plan(self, fn, fn_models, family, model, rs, model_index, run, rng_state, mpl=None, **dims):
        """The host call OLOP, BRUE and Sparse Sampling plans share: ``fn(ctx, model, n, roots, *run, rng, [mpl], results,
        MP_MEM_HOST)``, or ``fn_models`` with ``model_index`` (one MDP per root) in front of the roots -> the result dict.
        ``dims``: the family's other trailing dimensions."""
        n = rs.shape[0]
        out = _results(family, n, **({} if mpl is None else {"L": mpl}), **dims)
        roots = (n, _ptr(rs))
        if model_index is not None:
            fn, roots = fn_models, (n, _ptr(np.ascontiguousarray(model_index, dtype=np.int32).reshape(n)), _ptr(rs))
        _check(fn(self._h, model._h, *roots, *run, _ptr(rng_state), *(() if mpl is None else (mpl,)), *_result_ptrs(family, out),
                  MP_MEM_HOST))
        return out

    def olop_plan(self, model, root_state, episodes, horizon, gamma, kl, continuation, thresholds, value_upper_init, rng_state,
                  max_plan_len=None, model_index=None):
        """OLOP.plan for a batch of roots (host arrays): mp_olop_plan.  ``kl``: the kullback-leibler bound (else mu_ucb stays
        inf); ``continuation``: < 0 = uniform, else the action label taken after an expansion; ``thresholds`` float64
        [episodes], ``value_upper_init`` float64 [horizon + 1] from the host.  ``model_index`` int [n]: a batch model with one
        MDP per root, ``root_state`` local (mp_olop_plan_models)."""
        return self._olop_plan(self._lib.mp_olop_plan, self._lib.mp_olop_plan_models, "olop_plan", model, root_state, episodes,
                               horizon, gamma, kl, continuation, thresholds, value_upper_init, rng_state, max_plan_len, model_index)

    def olop_plan_stochastic(self, model, root_state, episodes, horizon, gamma, kl, continuation, thresholds, value_upper_init,
                             rng_state, max_plan_len=None):
        """OLOP.plan on a ``stochastic`` / ``sparse`` model for a batch of roots (host arrays): mp_olop_plan_stochastic.
        Arguments and results as :meth:`olop_plan`; the clone is re-seeded per episode from the planner's draw and every model
        step samples the model's row with the clone's own generator.  :meth:`olop_tree` serves the trees afterwards."""
        return self._olop_plan(self._lib.mp_olop_plan_stochastic, None, "olop_plan_stochastic", model, root_state, episodes,
                               horizon, gamma, kl, continuation, thresholds, value_upper_init, rng_state, max_plan_len, None)

    def _olop_plan(self, fn, fn_models, name, model, root_state, episodes, horizon, gamma, kl, continuation, thresholds,
                   value_upper_init, rng_state, max_plan_len, model_index):
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        _check_rng(rng_state, rs.shape[0])
        mpl = max(int(horizon), 1) if max_plan_len is None else int(max_plan_len)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        vin = np.ascontiguousarray(value_upper_init, dtype=np.float64).reshape(-1)
        if vin.size != int(horizon) + 1 or (kl and thr.size < int(episodes)):
            raise ValueError("{}: thresholds [episodes] and value_upper_init [horizon + 1] expected".format(name))
        run = (int(episodes), int(horizon), float(gamma), 1 if kl else 0, int(continuation), _ptr(thr) if thr.size else None,
               _ptr(vin))
        return self._each_plan(fn, fn_models, "olop", model, rs, model_index, run, rng_state, mpl)

    OLOP_TREE = (("parent", np.int32, ()), ("action", np.int32, ()), ("depth", np.int32, ()), ("count", np.int64, ()),
                 ("cum", np.float64, ()), ("mu", np.float64, ()), ("vu", np.float64, ()), ("done", np.uint8, ()),
                 ("state", np.int32, ()))

    def olop_tree(self, root, cap):
        """Creation-order arrays of root ``root``'s tree after the last olop_plan (mp_olop_tree_export)."""
        return _export_tree(self._lib.mp_olop_tree_export, (self._h, int(root)), cap, self.OLOP_TREE)

    def gape_plan(self, model, root_state, episodes, horizon, gamma, accuracy, uniform, n_actions_env, action_column, thr_by_count,
                  value_init, rng_state, model_index=None):
        """MDPGapE.plan for a batch of roots (host arrays): mp_gape_plan.  ``uniform``: the "uniform" continuation (else action
        0 of the environment); ``action_column`` int [n_actions_env] or None: the model column of each environment action;
        ``thr_by_count`` float64 [episodes + 2] and ``value_init`` float64 [horizon + 1] from the host.  ``plans`` [n, 1]: the
        best arm's action (a column of the model), as ``best_challenger`` [n, 2]; ``child_*`` [n, A] by column.
        ``model_index`` int [n]: a batch model with one MDP per root, ``root_state`` local (mp_gape_plan_models)."""
        return self._gape_plan(self._lib.mp_gape_plan, self._lib.mp_gape_plan_models, "gape_plan", model, root_state, episodes,
                               horizon, gamma, accuracy, uniform, n_actions_env, action_column, thr_by_count, value_init, rng_state,
                               model_index=model_index)

    def _gape_plan(self, fn, fn_models, name, model, root_state, episodes, horizon, gamma, accuracy, uniform, n_actions_env,
                   action_column, thr_by_count, value_init, rng_state, transition_thr_by_count=None, max_next_states=None,
                   model_index=None):
        """gape_plan and, with ``transition_thr_by_count`` and ``max_next_states``, gape_plan_stochastic."""
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        _check_rng(rng_state, rs.shape[0])
        stochastic = max_next_states is not None
        thr = np.ascontiguousarray(thr_by_count, dtype=np.float64).reshape(-1)
        tthr = np.ascontiguousarray(transition_thr_by_count, dtype=np.float64).reshape(-1) if stochastic else None
        vin = np.ascontiguousarray(value_init, dtype=np.float64).reshape(-1)
        if vin.size != int(horizon) + 1 or any(t.size != int(episodes) + 2 for t in ((thr, tthr) if stochastic else (thr,))):
            raise ValueError("{}: thr_by_count {}[episodes + 2] and value_init [horizon + 1] expected".format(
                name, "and transition_thr_by_count " if stochastic else ""))
        col = None if action_column is None else np.ascontiguousarray(action_column, dtype=np.int32).reshape(-1)
        if col is not None and col.size != int(n_actions_env):
            raise ValueError("{}: action_column [n_actions_env] expected".format(name))
        shared = (float(gamma), float(accuracy), 1 if uniform else 0, int(n_actions_env), _ptr(col), _ptr(thr))
        if stochastic:
            run = (int(episodes), int(horizon), int(max_next_states)) + shared + (_ptr(tthr), _ptr(vin))
        else:
            run = (int(episodes), int(horizon)) + shared + (_ptr(vin),)
        return self._each_plan(fn, fn_models, "gape", model, rs, model_index, run, rng_state, 1, A=model.A, P=2)

    GAPE_TREE = (("kind", np.uint8, ()), ("parent", np.int32, ()), ("action", np.int32, ()), ("depth", np.int32, ()),
                 ("count", np.int64, ()), ("cum", np.float64, ()), ("mu_ucb", np.float64, ()), ("mu_lcb", np.float64, ()),
                 ("vu", np.float64, ()), ("vl", np.float64, ()), ("done", np.uint8, ()), ("state", np.int32, ()))

    def gape_tree(self, root, cap=None):
        """Creation-order arrays of root ``root``'s tree after the last gape_plan, decision (``kind`` 0) and chance (1) nodes
        (mp_gape_tree_export).  ``cap`` None: the tree's own node count is asked first."""
        return self._gape_tree(self._lib.mp_gape_tree_export, root, cap)

    def _gape_tree(self, fn, root, cap):
        if cap is None:
            n = c_i32()
            rc = fn(self._h, int(root), 0, C.byref(n), *([None] * len(self.GAPE_TREE)))
            if n.value < 1:                                     # (no tree to size: the refusal itself)
                _check(rc)
            cap = n.value
        return _export_tree(fn, (self._h, int(root)), cap, self.GAPE_TREE)

    def gape_plan_stochastic(self, model, root_state, episodes, horizon, max_next_states, gamma, accuracy, uniform, n_actions_env,
                             action_column, thr_by_count, transition_thr_by_count, value_init, rng_state):
        """MDPGapE.plan with ``max_next_states_count`` = ``max_next_states`` in 1..32 on a deterministic table, a dense or a
        sparse model, for a batch of roots (host arrays): mp_gape_plan_stochastic.  Arguments and results as :meth:`gape_plan`,
        and ``transition_thr_by_count`` float64 [episodes + 2]: ``transition_threshold()`` by a chance node's count.
        ``status`` ERR_GAPE_PLACEHOLDERS where more next states were observed than placeholders.  :meth:`gape_stoch_tree`
        serves the trees afterwards.  (One MDP per root: :meth:`gape_plan_stochastic_models`.)"""
        return self._gape_plan(self._lib.mp_gape_plan_stochastic, None, "gape_plan_stochastic", model, root_state, episodes, horizon,
                               gamma, accuracy, uniform, n_actions_env, action_column, thr_by_count, value_init, rng_state,
                               transition_thr_by_count=transition_thr_by_count, max_next_states=max_next_states)

    def gape_plan_stochastic_models(self, model, model_index, root_state, episodes, horizon, max_next_states, gamma, accuracy, uniform,
                                    n_actions_env, action_column, thr_by_count, transition_thr_by_count, value_init, rng_state):
        """:meth:`gape_plan_stochastic` on a batch model of deterministic tables with one MDP per root
        (mp_gape_plan_stochastic_models): ``model_index`` int [n], ``root_state`` local to the MDP it names; the remaining
        arguments and the results are those of :meth:`gape_plan_stochastic`.  :meth:`gape_stoch_tree` serves the trees
        afterwards, with global states.  (A method of its own, not a keyword of :meth:`gape_plan_stochastic`: that method's
        signature is part of what the recorded planner calls pin.)"""
        if model_index is None:
            raise ValueError("gape_plan_stochastic_models: model_index [n] expected")
        return self._gape_plan(None, self._lib.mp_gape_plan_stochastic_models, "gape_plan_stochastic_models", model, root_state,
                               episodes, horizon, gamma, accuracy, uniform, n_actions_env, action_column, thr_by_count, value_init,
                               rng_state, transition_thr_by_count=transition_thr_by_count, max_next_states=max_next_states,
                               model_index=model_index)

    def gape_stoch_tree(self, root, cap=None):
        """BREADTH-FIRST arrays of root ``root``'s tree after the last gape_plan_stochastic, children in the reference's dict
        order, with the fields of :meth:`gape_tree` (mp_gape_stoch_tree_export): the ``action`` of a decision node is its
        observed state, or ``-1 - i`` for ``placeholder_i``.  ``cap`` None: the tree's own node count is asked first."""
        return self._gape_tree(self._lib.mp_gape_stoch_tree_export, root, cap)

    def selftest_gape_transition(self, f, q, c):
        """What the DEVICE computes for ``max_expectation_under_constraint`` (mp_selftest_gape_transition): ``f``, ``q`` float64
        [n, K], ``c`` float64 [n] -> (p_star [n, K], Newton iterations int32 [n], decisions int32 [n]: the KT_* bits of
        csrc/kl_transition.hpp)."""
        f = np.ascontiguousarray(f, dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
        if f.ndim != 2 or q.shape != f.shape or c.size != f.shape[0]:
            raise ValueError("selftest_gape_transition: f, q [n, K] and c [n] expected")
        p_star = np.zeros(f.shape, np.float64)
        its, mask = np.zeros(c.size, np.int32), np.zeros(c.size, np.int32)
        _check(self._lib.mp_selftest_gape_transition(self._h, f.shape[0], f.shape[1], _ptr(f), _ptr(q), _ptr(c), _ptr(p_star),
                                                     _ptr(its), _ptr(mask)))
        return p_star, its, mask

    def brue_plan(self, model, root_state, budget, horizon, gamma, gpow, rng_state, model_index=None):
        """BRUE.plan for a batch of roots (host arrays): mp_brue_plan.  ``gpow`` float64 [horizon + 1]: gamma ** d from the
        host.  ``plans`` [n]: the one planned action per root (-1 where no rollout was made).  ``model_index`` int [n]: a batch
        model with one MDP per root, ``root_state`` local (mp_brue_plan_models)."""
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        _check_rng(rng_state, rs.shape[0])
        gp = np.ascontiguousarray(gpow, dtype=np.float64).reshape(-1)
        if gp.size != int(horizon) + 1:
            raise ValueError("brue_plan: gpow [horizon + 1] expected")
        return self._each_plan(self._lib.mp_brue_plan, self._lib.mp_brue_plan_models, "brue", model, rs, model_index,
                               (int(budget), int(horizon), float(gamma), _ptr(gp)), rng_state)

    BRUE_TREE = (("parent", np.int32, ()), ("key", np.int32, ()), ("is_chance", np.uint8, ()), ("depth", np.int32, ()),
                 ("count", np.int64, ()), ("stat", np.float64, ()))

    def brue_tree(self, root, cap):
        """Creation-order arrays of root ``root``'s tree after the last brue_plan (mp_brue_tree_export)."""
        return _export_tree(self._lib.mp_brue_tree_export, (self._h, int(root)), cap, self.BRUE_TREE)

    def ss_plan(self, model, root_state, horizon, C, gamma, rng_state, model_index=None):
        """SparseSampling.plan for a batch of roots (host arrays): mp_ss_plan.  ``plans`` [n]: the one planned action per
        root (a column of the model); ``samples`` [n]: model steps taken.  ``model_index`` int [n]: a batch model with one
        MDP per root, ``root_state`` local (mp_ss_plan_models)."""
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        _check_rng(rng_state, rs.shape[0])
        return self._each_plan(self._lib.mp_ss_plan, self._lib.mp_ss_plan_models, "ss", model, rs, model_index,
                               (int(horizon), int(C), float(gamma)), rng_state)

    SS_TREE = (("parent", np.int32, ()), ("key", np.int32, ()), ("is_chance", np.uint8, ()), ("depth", np.int32, ()),
               ("count", np.int64, ()), ("value", np.float64, ()))

    def ss_tree(self, root, cap=None):
        """Creation-order arrays of root ``root``'s tree after the last ss_plan (mp_ss_tree_export).  ``cap`` None: the
        tree's own node count is asked first."""
        if cap is None:
            n = c_i32()
            rc = self._lib.mp_ss_tree_export(self._h, int(root), 0, C.byref(n), None, None, None, None, None, None)
            if n.value < 1:                                     # (no tree to size: the refusal itself)
                _check(rc)
            cap = n.value
        return _export_tree(self._lib.mp_ss_tree_export, (self._h, int(root)), cap, self.SS_TREE)


class PinnedArrays(dict):
    """``{name: ndarray}`` views of one pinned host allocation (mp_host_alloc); 64-byte aligned members."""

    def __init__(self, ctx, spec):
        super(PinnedArrays, self).__init__()
        self.ctx = ctx
        offs, total = {}, 0
        for name, (shape, dtype) in spec.items():
            offs[name] = total
            total += (int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize + 63) & ~63
        self._ptr = _vp()
        _check(ctx._lib.mp_host_alloc(ctx._h, max(total, 64), C.byref(self._ptr)))
        self.nbytes = total
        raw = np.ctypeslib.as_array((C.c_uint8 * max(total, 64)).from_address(self._ptr.value))
        for name, (shape, dtype) in spec.items():
            n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            self[name] = raw[offs[name]:offs[name] + n].view(dtype).reshape(shape)

    def close(self):
        if getattr(self, "_ptr", None) is not None and getattr(self.ctx, "_h", None):
            self.clear()
            self.ctx._lib.mp_host_free(self.ctx._h, self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceRng(_Handle):
    """numpy-PCG64 generator records of a batch of roots, resident on the device (mp_rng): the planners advance them in
    place and nothing crosses PCIe until ``get`` is asked for."""
    _free = "mp_rng_free"

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        self._h = _vp()
        _check(ctx._lib.mp_rng_create(ctx._h, self.n, C.byref(self._h)))

    def set(self, states, first=0):
        st = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 6)
        _check(self.ctx._lib.mp_rng_set(self._h, int(first), st.shape[0], _ptr(st)))

    def get(self, first=0, count=None):
        count = self.n - int(first) if count is None else int(count)
        out = np.zeros((count, 6), dtype=np.uint64)
        _check(self.ctx._lib.mp_rng_get(self._h, int(first), count, _ptr(out)))
        return out

    def seed_sequence(self, entropy, first_key=0, first=0, count=None):
        """Record first + i <- Generator(PCG64(SeedSequence(list(entropy) + [first_key + i]))) (see seed_sequence_states)."""
        count = self.n - int(first) if count is None else int(count)
        w = entropy_words(entropy) if not (hasattr(entropy, "__len__") and len(entropy) == 0) else np.zeros(0, np.uint32)
        _check(self.ctx._lib.mp_rng_seed_sequence(self._h, int(first), count, _ptr(w) if len(w) else None, len(w),
                                                  int(first_key)))

    def ptr(self, first=0):
        p = self.ctx._lib.mp_rng_device_ptr(self._h, int(first))
        if not p:
            raise NativeError(MP_ERR_ARG, load().mp_last_error().decode("utf-8", "replace"))
        return p



class Model(_Handle):
    """Device-resident transition model (mp_model)."""
    _free = "mp_model_free"

    def __init__(self, ctx, handle, mode, m, s, a, b):
        self.ctx, self._h, self.mode, self.M, self.S, self.A, self.B = ctx, handle, mode, m, s, a, b
        self._keep = None
        self.n_models, self.S_each = 1, s       # batch models (Context.load_table_batch): N MDPs of S_each states

    def set_available(self, available):
        """Restrict the action sets (mp_model_set_available): bool [S, A] over this model's (global) states."""
        av = _flags(available, self.S, self.A)
        _check(self.ctx._lib.mp_model_set_available(self._h, _ptr(av)))
        self.available = av.astype(bool)

    def update_tables(self, first, transition, reward, terminal=None):
        """Replace the tables of MDPs [first, first + count) of a batch model -- or the whole of a single table model with
        first = 0 -- (mp_model_update_tables): transition int [count,S,A] LOCAL states, reward [count,S,A], terminal
        [count,S] iff the model has terminal flags.  Stream-ordered, no synchronisation; policies loaded for the model
        become invalid."""
        t = np.ascontiguousarray(transition, dtype=np.int64).reshape(-1, self.S_each, self.A)
        r = np.ascontiguousarray(reward, dtype=np.float64).reshape(t.shape)
        term = _flags(terminal, t.shape[0], self.S_each)
        _check(self.ctx._lib.mp_model_update_tables(self._h, int(first), int(t.shape[0]), _ptr(t), _ptr(r), _ptr(term)))

    def update_rows(self, rows, transition, reward, terminal=None):
        """Delta upload (mp_model_update_rows): rows int [k] GLOBAL state ids (distinct), transition int [k,A] LOCAL next
        states of each row's MDP, reward [k,A], terminal [k] or None = the rows' flags do not change."""
        rw = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(transition, dtype=np.int64).reshape(rw.shape[0], self.A)
        r = np.ascontiguousarray(reward, dtype=np.float64).reshape(t.shape)
        term = _flags(terminal, rw.shape[0])
        if len(np.unique(rw)) != len(rw):
            raise ValueError("update_rows: row ids must be distinct")
        _check(self.ctx._lib.mp_model_update_rows(self._h, int(rw.shape[0]), _ptr(rw), _ptr(t), _ptr(r), _ptr(term)))

    def set_episode_rules(self, done_rule="source", max_steps=0):
        """Terminal convention and TimeLimit of the env stepping this model (dense / sparse models: table models get them
        at load time)."""
        _check(self.ctx._lib.mp_model_set_episode_rules(self._h, int(done_rule == "next"), int(max_steps or 0)))



class JointBatchModel(Model):
    """N sets of M deterministic tables (mp_model_load_joint_batch): ``n_models`` sets, ``M`` models a set, ``S_each`` states a
    table; ``S`` counts the N * S_each global states."""

    def set_available(self, available):
        """What each model's env lists in get_available_actions(): bool [N, M, S, A] (mp_model_set_available_joint_batch).
        The flags survive :meth:`update_tables`."""
        av = _flags(available, self.n_models, self.M, self.S_each, self.A)
        _check(self.ctx._lib.mp_model_set_available_joint_batch(self._h, _ptr(av)))
        self.available = av.astype(bool)

    def update_tables(self, first, transition, reward, terminal=None):
        """Replace sets [first, first + count) (mp_model_update_joint_tables): transition int [count,M,S,A] LOCAL next
        states, reward [count,M,S,A], terminal [count,M,S] iff the model has terminal flags.  Stream-ordered."""
        t = np.ascontiguousarray(transition, dtype=np.int64).reshape(-1, self.M, self.S_each, self.A)
        r = np.ascontiguousarray(reward, dtype=np.float64).reshape(t.shape)
        term = _flags(terminal, t.shape[0], self.M, self.S_each)
        _check(self.ctx._lib.mp_model_update_joint_tables(self._h, int(first), int(t.shape[0]), _ptr(t), _ptr(r), _ptr(term)))


class StateAwarePlanners(_Handle):
    """A batch of device-resident StateAwarePlanner objects (mp_saopd): state values, state-node lists and the node
    arena persist across plan() calls, as in the reference (tree_search/state_aware.py:76-83)."""
    _free = "mp_saopd_free"

    def __init__(self, ctx, model, n_planners):
        self.ctx, self.model, self.n = ctx, model, int(n_planners)
        self._h = _vp()
        _check(ctx._lib.mp_saopd_create(ctx._h, model._h, self.n, C.byref(self._h)))

    def plan(self, root_state, budget, gamma, terminal_reward, rng_state, accuracy=0.0, backup_aggregated_nodes=True,
             prune_suboptimal_leaves=True, max_plan_len=None):
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        if rs.shape[0] != self.n:
            raise ValueError("one root state per planner ({}), got {}".format(self.n, rs.shape[0]))
        _check_rng(rng_state, self.n, "n_planners")
        mpl = int(budget + 1 if max_plan_len is None else max_plan_len)
        out = _results("saopd", self.n, L=mpl)
        self._call(MP_MEM_HOST, _ptr(rs), budget, gamma, terminal_reward, accuracy, backup_aggregated_nodes,
                   prune_suboptimal_leaves, _ptr(rng_state), mpl, _result_ptrs("saopd", out))
        return out

    def _call(self, mem, rs, budget, gamma, terminal_reward, accuracy, backup_aggregated_nodes, prune_suboptimal_leaves, rng, mpl,
              o):
        """The one call of mp_saopd_plan, on addresses (``o``: those of the five results)."""
        _check(self.ctx._lib.mp_saopd_plan(self.ctx._h, self._h, rs, int(budget), float(gamma), float(terminal_reward),
                                           float(accuracy), int(bool(backup_aggregated_nodes)),
                                           int(bool(prune_suboptimal_leaves)), rng, int(mpl), *o, mem))

    def plan_device(self, root_state, budget, gamma, terminal_reward, rng_state, max_plan_len, accuracy=0.0,
                    backup_aggregated_nodes=True, prune_suboptimal_leaves=True, plans=None, plan_len=None, env_steps=None,
                    updates=None, status=None):
        """Asynchronous form: every array is a device buffer (torch tensors on the context's device: root_state int32
        [n], rng_state uint64-as-int64 [n, 6], plans int32 [n, max_plan_len], plan_len / status int32 [n], env_steps /
        updates int64 [n]); one launch on the context's stream, nothing read back.  A planner whose backup queue fills up
        reports MP_ERR_ALLOC in ``status`` and stays failed for every later call (mi355plan.h)."""
        self._call(MP_MEM_DEVICE, _ptr(root_state), budget, gamma, terminal_reward, accuracy, backup_aggregated_nodes,
                   prune_suboptimal_leaves, _ptr(rng_state), max_plan_len, _ptrs(plans, plan_len, env_steps, updates, status))

    def info(self):
        n, nn, root, s = c_i32(), c_i32(), c_i32(), c_i32()
        _check(self.ctx._lib.mp_saopd_info(self._h, C.byref(n), C.byref(nn), C.byref(root), C.byref(s)))
        return dict(n_planners=n.value, n_nodes=nn.value, root=root.value, n_states=s.value)

    ARENA = (("parent", np.int32, ()), ("action", np.int32, ()), ("state", np.int32, ()), ("depth", np.int32, ()),
             ("reward", np.float64, ()), ("lower", np.float64, ()), ("done", np.uint8, ()), ("count", np.int64, ()),
             ("first_child", np.int32, ()), ("alive", np.uint8, ()))

    def export(self, planner=0, current_tree_only=True):
        """Arena of one planner; current_tree_only: the nodes of the last plan's tree, ids re-based at its root."""
        inf = self.info()
        cap = inf["n_nodes"]
        t = _zeros(cap, self.ARENA)
        sv = np.zeros(inf["n_states"], np.float64)
        _check(self.ctx._lib.mp_saopd_export(self._h, int(planner), cap, *(_ptrs(*t.values()) + [_ptr(sv)])))
        # Rows of actions the environment does not list (restricted action sets, deterministic.py:32-35) are PHANTOMS in
        # the arena -- lower = -inf, never alive -- that only keep the ids of an expansion's |A| slots contiguous: they
        # are not nodes of the tree.  Drop them and renumber; a node's children are then contiguous from first_child,
        # n_children of them.
        lo = inf["root"] if current_tree_only else 0
        keep = ~np.isneginf(t["lower"])
        new_id = np.cumsum(keep) - 1
        a = self.model.A
        fc_old = t["first_child"].copy()
        has = fc_old >= 0
        # an expansion's |A| slots fc .. fc + |A| - 1: how many are real nodes, and the first of them
        csum = np.concatenate([[0], np.cumsum(keep)])
        fc0 = np.where(has, fc_old, 0)
        n_children = np.where(has, csum[np.minimum(fc0 + a, cap)] - csum[fc0], 0).astype(np.int32)
        next_kept = np.where(keep, np.arange(cap), cap)
        next_kept = np.minimum.accumulate(next_kept[::-1])[::-1] if cap else next_kept      # first kept row at or after i
        first_kept = np.where(n_children > 0, next_kept[fc0], -1)      # (every slot a phantom: no children, no first child)
        t["first_child"] = first_kept.astype(np.int32)
        t["n_children"] = n_children
        sel = keep.copy()
        sel[:lo] = False
        base = int(new_id[lo]) if lo < cap else 0
        out = {k: v[sel].copy() for k, v in t.items()}
        for k in ("parent", "first_child"):
            out[k] = np.where(out[k] >= lo, new_id[np.maximum(out[k], 0)] - base, -1).astype(np.int32)
        return out, sv



class _GraphPlanners(_Handle):
    """What the batches of mp_gbopd and of mp_gbop planners share: a host-array plan's checks and an export's reshaping."""

    def _roots_and_rng(self, root_state, rng_state):
        rs = np.ascontiguousarray(root_state, dtype=np.int32).reshape(-1)
        if rs.shape[0] != self.n:
            raise ValueError("one root state per planner ({}), got {}".format(self.n, rs.shape[0]))
        _check_rng(rng_state, self.n, "n_planners")
        return rs

    @staticmethod
    def _listed_first(listed, A):
        """-> n_children and ``take(x, fill)``: x [n, A, ...] with every node's listed slots first, in slot order, then ``fill``."""
        rank = np.argsort(~listed, axis=1, kind="stable")
        n_children = listed.sum(axis=1).astype(np.int32)
        keep = np.arange(A)[None, :] < n_children[:, None]

        def take(x, fill):
            tail = (1,) * (x.ndim - 2)
            idx = np.broadcast_to(rank.reshape(rank.shape + tail), x.shape)
            return np.where(keep.reshape(keep.shape + tail), np.take_along_axis(x, idx, axis=1), fill)
        return n_children, take


class GraphBasedPlanners(_GraphPlanners):
    """A batch of device-resident GraphBasedPlanner objects (mp_gbopd): the graph of observed states with both bounds, the
    parents in insertion order and the lifetime visit / update counters persist across plan() calls, as in the reference
    (tree_search/graph_based.py:87-94).  ``queue_cap``: entries of a planner's backup queue (None: the library's default)."""
    _free = "mp_gbopd_free"

    def __init__(self, ctx, model, n_planners, queue_cap=None):
        self.ctx, self.model, self.n = ctx, model, int(n_planners)
        self._h = _vp()
        _check(ctx._lib.mp_gbopd_create(ctx._h, model._h, self.n, int(queue_cap or 0), C.byref(self._h)))

    def plan(self, root_state, budget, gamma, value_max, accuracy, sampling_timeout, rng_state):
        """GraphBasedPlanner.plan for every planner (host arrays).  ``value_max``: the host's ``1 / (1 - gamma)``."""
        rs = self._roots_and_rng(root_state, rng_state)
        t = int(sampling_timeout)
        out = _results("gbopd", self.n, L=t)
        self._call(MP_MEM_HOST, _ptr(rs), budget, gamma, value_max, accuracy, t, _ptr(rng_state), _result_ptrs("gbopd", out))
        return out

    def _call(self, mem, rs, budget, gamma, value_max, accuracy, sampling_timeout, rng, o):
        """The one call of mp_gbopd_plan, on addresses (``o``: those of the seven results)."""
        _check(self.ctx._lib.mp_gbopd_plan(self.ctx._h, self._h, rs, int(budget), float(gamma), float(value_max),
                                           float(accuracy), int(sampling_timeout), rng, *o, mem))

    def plan_device(self, root_state, budget, gamma, value_max, accuracy, sampling_timeout, rng_state, plans=None,
                    plan_len=None, value_lower=None, value_upper=None, env_steps=None, updates=None, status=None):
        """Asynchronous form: every array is a device buffer (torch tensors on the context's device: root_state int32 [n],
        rng_state uint64-as-int64 [n, 6], plans int32 [n, sampling_timeout], plan_len / status int32 [n], value_lower /
        value_upper float64 [n], env_steps / updates int64 [n]); one launch on the context's stream, nothing read back."""
        self._call(MP_MEM_DEVICE, _ptr(root_state), budget, gamma, value_max, accuracy, sampling_timeout, _ptr(rng_state),
                   _ptrs(plans, plan_len, value_lower, value_upper, env_steps, updates, status))

    def info(self):
        n, s, a, q, e = c_i32(), c_i32(), c_i32(), c_i32(), c_i64()
        _check(self.ctx._lib.mp_gbopd_info(self._h, C.byref(n), C.byref(s), C.byref(a), C.byref(q), C.byref(e)))
        return dict(n_planners=n.value, n_states=s.value, n_actions=a.value, queue_cap=q.value, n_edges=e.value)

    def export(self, planner=0):
        """One planner's graph in creation order, in the fields of the goldens' listing: state, lower, upper, expanded,
        n_children, child_action / child_node / child_reward [n, A] (the listed actions first, in the model's slot order,
        -1 / 0 padded), parent_ptr / parent_idx, visits / updates [S], n_observations, root."""
        inf = self.info()
        S, A = inf["n_states"], inf["n_actions"]
        nn, nobs, root = c_i32(), c_i64(), c_i32()
        state, lower, upper = np.zeros(S, np.int32), np.zeros(S, np.float64), np.zeros(S, np.float64)
        expanded, child, reward = np.zeros(S, np.uint8), np.full((S, A), -1, np.int32), np.zeros((S, A), np.float64)
        pptr, pidx = np.zeros(S + 1, np.int32), np.zeros(max(inf["n_edges"], 1), np.int32)
        visits, updates = np.zeros(S, np.int64), np.zeros(S, np.int64)
        _check(self.ctx._lib.mp_gbopd_export(self._h, int(planner), S, C.byref(nn), _ptr(state), _ptr(lower), _ptr(upper),
                                             _ptr(expanded), _ptr(child), _ptr(reward), _ptr(pptr), _ptr(pidx), _ptr(visits),
                                             _ptr(updates), C.byref(nobs), C.byref(root)))
        n = nn.value
        child, reward = child[:n], reward[:n]
        n_children, take = self._listed_first(child >= 0, A)
        slots = np.broadcast_to(np.arange(A, dtype=np.int32), (n, A))
        return dict(state=state[:n].copy(), lower=lower[:n].copy(), upper=upper[:n].copy(), expanded=expanded[:n].copy(),
                    n_children=n_children, child_action=take(slots, -1).astype(np.int32),
                    child_node=take(child, -1).astype(np.int32), child_reward=take(reward, 0.0),
                    parent_ptr=pptr[:n + 1].copy(), parent_idx=pidx[:pptr[n]].copy(), visits=visits, updates=updates,
                    n_observations=np.asarray(nobs.value), root=np.asarray(root.value))


class StochasticGraphBasedPlanners(_GraphPlanners):
    """A batch of device-resident StochasticGraphBasedPlanner objects (mp_gbop): the graph of observed states with both
    bounds, counts and parents in insertion order, and per (state, listed action) the chance record with its
    ``max_next_states`` transition children persist across plan() calls, as in the reference
    (tree_search/graph_based_stochastic.py:339-343).  ``queue_cap``: entries of a planner's backup queue (None: the library's
    default)."""
    _free = "mp_gbop_free"
    # mp_gbop_export's arrays after n_nodes: (name, dtype, trailing shape in terms of A and K); then visits [S]
    EXPORT = (("state", np.int32, ""), ("lower", np.float64, ""), ("upper", np.float64, ""), ("expanded", np.uint8, ""),
              ("count", np.int64, ""), ("listed", np.uint8, "A"), ("chance_count", np.int32, "A"), ("chance_assigned", np.int32, "A"),
              ("chance_backed", np.int32, "A"), ("chance_value", np.float64, "A2"), ("child_state", np.int32, "AK"),
              ("child_count", np.int32, "AK"), ("child_cum", np.float64, "AK"), ("child_mu_ucb", np.float64, "AK"),
              ("child_mu_lcb", np.float64, "AK"), ("p_plus", np.float64, "AK"), ("p_minus", np.float64, "AK"))

    def __init__(self, ctx, model, n_planners, max_next_states, queue_cap=None):
        self.ctx, self.model, self.n, self.K = ctx, model, int(n_planners), int(max_next_states)
        self._h = _vp()
        _check(ctx._lib.mp_gbop_create(ctx._h, model._h, self.n, self.K, int(queue_cap or 0), C.byref(self._h)))

    def plan(self, root_state, episodes, horizon, gamma, value_max, accuracy, sampling_timeout, reward_thr_by_count,
             transition_thr_by_count, rng_state):
        """StochasticGraphBasedPlanner.plan for every planner (host arrays).  ``value_max``: the host's ``1 / (1 - gamma)``;
        the two threshold tables by LIFETIME count, ``[count - 1]``, at least ``info()["max_count"] + episodes * horizon``
        entries each."""
        rs = self._roots_and_rng(root_state, rng_state)
        out = _results("gbop", self.n)
        self._call(MP_MEM_HOST, _ptr(rs), episodes, horizon, gamma, value_max, accuracy, sampling_timeout, reward_thr_by_count,
                   transition_thr_by_count, _ptr(rng_state), _result_ptrs("gbop", out))
        return out

    def _call(self, mem, rs, episodes, horizon, gamma, value_max, accuracy, sampling_timeout, rthr, tthr, rng, o):
        """The one call of mp_gbop_plan, on addresses (``o``: those of the eight results)."""
        rthr = np.ascontiguousarray(rthr, dtype=np.float64).reshape(-1)
        tthr = np.ascontiguousarray(tthr, dtype=np.float64).reshape(-1)
        if rthr.size != tthr.size:
            raise ValueError("the reward and the transition threshold table must hold the same counts")
        _check(self.ctx._lib.mp_gbop_plan(self.ctx._h, self._h, rs, int(episodes), int(horizon), self.K, float(gamma),
                                          float(value_max), float(accuracy), int(sampling_timeout), int(rthr.size), _ptr(rthr),
                                          _ptr(tthr), rng, *o, mem))

    def plan_device(self, root_state, episodes, horizon, gamma, value_max, accuracy, sampling_timeout, reward_thr_by_count,
                    transition_thr_by_count, rng_state, action=None, key=None, plan_len=None, value_lower=None, value_upper=None,
                    env_steps=None, pops=None, status=None, rng_device_only=False):
        """Asynchronous form: every array is a device buffer (torch tensors on the context's device) but the two threshold
        tables, which stay host arrays; one launch on the context's stream, nothing read back.  ``rng_device_only``: the
        root states and results are host arrays and only ``rng_state`` lives on the device (MP_MEM_RNG_DEVICE)."""
        self._call(MP_MEM_RNG_DEVICE if rng_device_only else MP_MEM_DEVICE, _ptr(root_state), episodes, horizon, gamma, value_max,
                   accuracy, sampling_timeout, reward_thr_by_count, transition_thr_by_count, _ptr(rng_state),
                   _ptrs(action, key, plan_len, value_lower, value_upper, env_steps, pops, status))

    def info(self):
        n, s, a, k, q, e, c = c_i32(), c_i32(), c_i32(), c_i32(), c_i32(), c_i64(), c_i64()
        _check(self.ctx._lib.mp_gbop_info(self._h, C.byref(n), C.byref(s), C.byref(a), C.byref(k), C.byref(q), C.byref(e),
                                          C.byref(c)))
        return dict(n_planners=n.value, n_states=s.value, n_actions=a.value, max_next_states=k.value, queue_cap=q.value,
                    n_edges=e.value, max_count=c.value)

    def export(self, planner=0):
        """One planner's graph in creation order, in the fields of the goldens' listing (tests/gbop_restatement.py): state,
        lower, upper, expanded, count, n_children; per listing position [n, A]: action (the model's slot), c_count, c_upper,
        c_lower, c_backed; per child in the reference's DICT order [n, A, K]: k_state (-1 - i for ``placeholder_i``), k_count,
        k_cum, k_mu_ucb, k_mu_lcb; p_plus / p_minus as their backup wrote them; parent_ptr / parent_idx, visits [S],
        n_observations, root."""
        inf = self.info()
        S, A, K = inf["n_states"], inf["n_actions"], inf["max_next_states"]
        tails = {"": (), "A": (A,), "A2": (A, 2), "AK": (A, K)}
        t = {k: np.zeros((S,) + tails[tail], dtype) for k, dtype, tail in self.EXPORT}
        pptr, pidx = np.zeros(S + 1, np.int32), np.zeros(max(inf["n_edges"], 1), np.int32)
        visits = np.zeros(S, np.int64)
        nn, nobs, root = c_i32(), c_i64(), c_i32()
        _check(self.ctx._lib.mp_gbop_export(self._h, int(planner), S, C.byref(nn), *([_ptr(v) for v in t.values()] +
                                            [_ptr(pptr), _ptr(pidx), _ptr(visits), C.byref(nobs), C.byref(root)])))
        n = nn.value
        t = {k: v[:n] for k, v in t.items()}
        n_children, take = self._listed_first(t["listed"] != 0, A)
        # the reference's dict order of a chance node's children: the slots m .. K - 1, then 0 .. m - 1
        rot = (np.arange(K)[None, None, :] + t["chance_assigned"][:, :, None]) % K
        children = lambda x, fill: take(np.take_along_axis(x, rot, axis=2), fill)  # noqa: E731
        slots = np.broadcast_to(np.arange(A, dtype=np.int32), (n, A))
        return dict(state=t["state"].copy(), lower=t["lower"].copy(), upper=t["upper"].copy(), expanded=t["expanded"].copy(),
                    count=t["count"].copy(), n_children=n_children, action=take(slots, -1).astype(np.int32),
                    c_count=take(t["chance_count"], 0).astype(np.int64), c_upper=take(t["chance_value"][:, :, 0], 0.0),
                    c_lower=take(t["chance_value"][:, :, 1], 0.0), c_backed=take(t["chance_backed"], -1).astype(np.int32),
                    k_state=children(t["child_state"], 0).astype(np.int32), k_count=children(t["child_count"], 0).astype(np.int64),
                    k_cum=children(t["child_cum"], 0.0), k_mu_ucb=children(t["child_mu_ucb"], 0.0),
                    k_mu_lcb=children(t["child_mu_lcb"], 0.0), p_plus=take(t["p_plus"], 0.0), p_minus=take(t["p_minus"], 0.0),
                    parent_ptr=pptr[:n + 1].copy(), parent_idx=pidx[:pptr[n]].copy(), visits=visits,
                    n_observations=np.asarray(nobs.value), root=np.asarray(root.value))



class Policy(_Handle):
    """Device-resident per-state prior / rollout policy tables (mp_policy)."""
    _free = "mp_policy_free"

    def __init__(self, ctx, handle, model=None):
        self.ctx, self._h, self.model = ctx, handle, model      # keeps the model it is tied to alive



def check_device_sweeps(sweeps_out):
    """Raise if an asynchronous ``vi_solve_device`` reported failure (sweeps = -1); returns the sweep count."""
    n = int(sweeps_out.reshape(-1)[0].item())
    if n < 0:
        raise NativeError(MP_ERR_HIP, "value iteration failed on the device: the persistent kernel's grid was not "
                                      "resident (set MP_VI_NO_PERSIST=1 or use Context.vi_solve)")
    return n


def rng_state_from_generator(gen):
    """numpy Generator(PCG64) -> the 6 x uint64 state record the kernels step."""
    st = gen.bit_generator.state
    if st["bit_generator"] != "PCG64":
        raise ValueError("planner randomness must be a numpy PCG64 generator")
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = (1 << 64) - 1
    return np.array([s >> 64, s & m, inc >> 64, inc & m, st["has_uint32"], st["uinteger"]], dtype=np.uint64)


def generator_set_state(gen, state6):
    """Write a stepped 6 x uint64 record back into a numpy Generator (keeps host and device streams one)."""
    st = gen.bit_generator.state
    st["state"]["state"] = (int(state6[0]) << 64) | int(state6[1])
    st["state"]["inc"] = (int(state6[2]) << 64) | int(state6[3])
    st["has_uint32"] = int(state6[4])
    st["uinteger"] = int(state6[5])
    gen.bit_generator.state = st
