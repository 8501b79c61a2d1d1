"""The C ABI of include/mcbs.h as Python states it: its constants, ctypes mirrors of its structs (same field order, natural alignment) and
PROTOTYPES, the one table of its functions."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

ABI_VERSION = 1
DEFENDER_NONE, DEFENDER_SCAN_AND_REIMAGE, DEFENDER_EXTERNAL, DEFENDER_RANDOM_EVENTS = 0, 1, 2, 3
RNG_PHILOX, RNG_TAPE = 0, 1
# MCBS_TOPO_* (include/mcbs.h): what a topology's descriptors and node count make possible (mcbs_topology_traits, mcbs_step_topo_traits)
TOPO_ESCALATION, TOPO_LATERAL_EXPLOIT, TOPO_PRECONDITION, TOPO_PROBE, TOPO_MULTI_LEAK, TOPO_WIDE_ROWS = 1, 2, 4, 8, 16, 32
TOPO_ANY = 63
CATEGORICAL_MODES = {"sample": 0, "argmax": 1, "evaluate": 2}      # MCBS_CATEGORICAL_SAMPLE / _ARGMAX / _EVALUATE
CATEGORICAL_PHILOX_DOMAIN = 0xCA7E6041                              # MCBS_CATEGORICAL_PHILOX_DOMAIN
MCBS_MAX_ACTION_DIMS, MCBS_MULTICATEGORICAL_PHILOX_DOMAIN = 16, 0x3C47E6A1     # the MultiDiscrete head
MCBS_LINEAR_MAX_H, MCBS_LINEAR_GRAD_ROW_BLOCK = 512, 512                       # the masked action head from the latent and its gradient
MCBS_FIRST_LAYER_GRAD_ROW_BLOCK = 512                                          # the first layer from the observation: rows per block partial


class BatchCfg(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_envs", C.c_uint32), ("device", C.c_int32),
        ("maximum_node_count", C.c_uint32), ("maximum_total_credentials", C.c_uint32),
        ("maximum_discoverable_credentials_per_action", C.c_uint32),
        ("has_attacker_goal", C.c_uint32), ("goal_own_atleast", C.c_uint32),
        ("goal_reward", C.c_double), ("goal_low_availability", C.c_double), ("goal_own_atleast_percent", C.c_double),
        ("defender_goal_eviction", C.c_uint32), ("defender_kind", C.c_uint32),
        ("maintain_sla", C.c_double), ("winning_reward", C.c_double), ("losing_reward", C.c_double),
        ("scan_probability", C.c_double), ("scan_capacity", C.c_uint32), ("scan_frequency", C.c_uint32),
        ("auto_reset", C.c_uint32), ("max_episode_steps", C.c_uint32), ("rng_kind", C.c_uint32), ("reserved0", C.c_uint32),
        ("seed", C.c_uint64), ("env_id_base", C.c_uint64),
    ]


assert C.sizeof(BatchCfg) == 136


class ObsBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties",
        "nodes_privilegelevel", "mask_local", "mask_remote", "mask_connect", "mask_discrete")]


class WrapperBuffers(C.Structure):
    """mcbs_wrapper_buffers (include/mcbs.h): device arrays of AttackerEnvWrapper's per-env bookkeeping"""
    _fields_ = [(n, C.c_void_p) for n in ("invalid", "reward", "terminated", "timesteps", "valid_action_count", "invalid_action_count",
                                          "episode_returns", "last_cyber_reward", "has_cyber_reward", "rewards", "truncated", "dones",
                                          "episode_return_out", "episode_length_out", "n_done", "executed")]


class DefenderWrapperBuffers(C.Structure):
    """mcbs_defender_wrapper_buffers (include/mcbs.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("valid", "availability", "evicted", "attacker_has_cyber_reward", "attacker_last_cyber_reward",
                                          "timesteps", "valid_action_count", "invalid_action_count", "has_breached_sla", "prev_availability",
                                          "reward", "terminated", "truncated", "breached", "won")]


class DefenderWrapperCfg(C.Structure):
    _fields_ = [("invalid_action_penalty", C.c_double), ("loss_reward", C.c_double), ("sla_worsening_penalty_scale", C.c_double),
                ("maintain_sla", C.c_double), ("winning_reward", C.c_double), ("reset_on_constraint_broken", C.c_int32),
                ("max_timesteps", C.c_int32)]


class DefenderObs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("infected_nodes", "incoming_firewall_status", "outgoing_firewall_status", "services_status")]


# mcbs_episode_buffers (include/mcbs.h): six device pointers, these members in this order.  An array of six pointers, not a
# Structure: byref() hands over the same 48 bytes, and the Structures of this module are exactly those tests/test_native_library.py
# lists against the header — this block is held to the header by tests/test_two_agent_host.py.  Filled through episode_buffers()
EPISODE_FIELDS = ("alive", "attacker_reward", "defender_reward", "lengths", "attacker_done", "defender_done")
EpisodeBuffers = C.c_void_p * len(EPISODE_FIELDS)


def episode_buffers(**arrays) -> "EpisodeBuffers":
    """An mcbs_episode_buffers block from device pointers given by member name (every member of EPISODE_FIELDS)."""
    if set(arrays) != set(EPISODE_FIELDS):
        raise ValueError(f"mcbs_episode_buffers has exactly the members {EPISODE_FIELDS}")
    return EpisodeBuffers(*[arrays[n] for n in EPISODE_FIELDS])


# mcbs_training_buffers (include/mcbs.h): seventeen device pointers, these members in this order — an array of pointers like
# EpisodeBuffers, held to the header by tests/test_training_host.py.  Filled through training_buffers()
TRAINING_FIELDS = ("attacker_reset_request", "defender_return", "attacker_valid_out", "attacker_invalid_out", "defender_return_out",
                   "defender_length_out", "defender_valid_out", "defender_invalid_out", "defender_dones", "terminal_infected_nodes",
                   "terminal_incoming_firewall_status", "terminal_outgoing_firewall_status", "terminal_services_status",
                   "fresh_infected_nodes", "fresh_incoming_firewall_status", "fresh_outgoing_firewall_status", "fresh_services_status")
TrainingBuffers = C.c_void_p * len(TRAINING_FIELDS)


def training_buffers(**arrays) -> "TrainingBuffers":
    """An mcbs_training_buffers block from device pointers given by member name (every member of TRAINING_FIELDS)."""
    if set(arrays) != set(TRAINING_FIELDS):
        raise ValueError(f"mcbs_training_buffers has exactly the members {TRAINING_FIELDS}")
    return TrainingBuffers(*[arrays[n] for n in TRAINING_FIELDS])


# mcbs_training_packed_buffers (include/mcbs.h): the nine per-env members of mcbs_training_buffers, then the defender's terminal packed
# rows and its fresh packed row — eleven device pointers, held to the header by tests/test_training_packed_host.py
TRAINING_PACKED_FIELDS = TRAINING_FIELDS[:9] + ("terminal_defender_packed", "fresh_defender_packed")
TrainingPackedBuffers = C.c_void_p * len(TRAINING_PACKED_FIELDS)


def training_packed_buffers(**arrays) -> "TrainingPackedBuffers":
    """An mcbs_training_packed_buffers block from device pointers given by member name (every member of TRAINING_PACKED_FIELDS)."""
    if set(arrays) != set(TRAINING_PACKED_FIELDS):
        raise ValueError(f"mcbs_training_packed_buffers has exactly the members {TRAINING_PACKED_FIELDS}")
    return TrainingPackedBuffers(*[arrays[n] for n in TRAINING_PACKED_FIELDS])


class BatchVariantInfo(C.Structure):
    """mcbs_batch_variant_info (include/mcbs.h): the compiled variant a batch dispatches to"""
    _fields_ = [(n, C.c_uint32) for n in ("packed", "words_per_set", "wide", "coop", "lds_topo", "defender_kind", "fused_wrapper",
                                          "fused_defender_obs")]


class GaeIO(C.Structure):
    """mcbs_gae_io (include/mcbs.h): device pointers, sizes, row strides in elements and the two coefficients of mcbs_gae"""
    _fields_ = ([(n, C.c_void_p) for n in ("rewards", "values", "episode_starts", "bootstrap", "last_values", "last_dones", "advantages",
                                           "returns")]
                + [("n_steps", C.c_uint64), ("n_envs", C.c_uint64)]
                + [(n, C.c_size_t) for n in ("rewards_stride", "values_stride", "episode_starts_stride", "bootstrap_stride",
                                             "advantages_stride", "returns_stride")]
                + [("gamma", C.c_double), ("gae_lambda", C.c_double)])


assert C.sizeof(GaeIO) == 144


class InfoBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("network_availability", "step_count", "truncated", "out_of_bound", "raw_reward")]


class RowCopies(C.Structure):
    """mcbs_row_copies (include/mcbs.h): up to eight (src, dst, row_bytes) triples for mcbs_copy_rows_masked."""
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("src", C.c_void_p * 8), ("dst", C.c_void_p * 8), ("row_bytes", C.c_size_t * 8)]


# ---- the prototypes of include/mcbs.h: THE declaration of the C ABI on the Python side.  engine.load_library applies it, engine.EXPORTS is
# its keys, and tests/test_native_library.py holds every entry (and every struct and constant of this file) to the header.  A new entry
# point is bound by adding its line here, in the header's order, with the header's parameter names beside it. ----
_int, _i32, _u32, _u64, _size, _f32 = C.c_int, C.c_int32, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float
_H = C.c_void_p                    # a handle: mcbs_batch*, mcbs_topology*, mcbs_feature_layout*, mcbs_obs_packing*
_P = C.c_void_p                    # an array on the device or the host, or an argument block handed over with byref()
_S = C.c_void_p                    # void* stream (a hipStream_t)
_NEW = C.POINTER(C.c_void_p)       # mcbs_x** out: receives a new handle
_OBS, _INFO, _DOBS = C.POINTER(ObsBuffers), C.POINTER(InfoBuffers), C.POINTER(DefenderObs)
# logits, dtype, row_stride, mode, actions, log_prob, entropy, n_allowed, uniforms, seed, step, bad_actions, stream
_CAT = [_P, _i32, _size, _i32, _P, _P, _P, _P, _P, _u64, _u64, _P, _S]
# latent, latent_row_stride, weight, weight_row_stride, bias, H, dtype, mode, actions, log_prob, entropy, n_allowed, uniforms, seed, step,
# bad_actions, stream
_LIN = [_P, _size, _P, _size, _P, _u32, _i32, _i32, _P, _P, _P, _P, _P, _u64, _u64, _P, _S]
_BITS = [_H, _P, _size, _u64]      # batch, bits, bits_row_words, n_rows
# weight_t, weight_row_stride, bias, weight_dtype, H, out, out_dtype, out_row_stride, out_of_range, stream
_FL = [_P, _size, _P, _i32, _u32, _P, _i32, _size, _P, _S]

PROTOTYPES = {
    "mcbs_last_error": (C.c_char_p, []),
    "mcbs_abi_version": (_u32, []),
    "mcbs_topology_create": (_int, [_P, _size, _i32, _NEW]),                                  # blob, nbytes, device, out
    "mcbs_topology_destroy": (None, [_H]),
    "mcbs_batch_create": (_int, [_H, C.POINTER(BatchCfg), _NEW]),                             # topology, cfg, out
    "mcbs_batch_destroy": (None, [_H]),
    "mcbs_reset": (_int, [_H, _P, _S]),                                                       # batch, env_mask, stream
    "mcbs_rewind": (_int, [_H, _S]),
    "mcbs_step": (_int, [_H, _P, _P, _P, _INFO, _S]),                                         # batch, actions, reward, terminated, info, stream
    "mcbs_step_many": (_int, [_H, _P, _P, _P, _u32, _S]),                                     # batch, actions, reward, terminated, n_steps, stream
    # batch, valid, seed, first_step, n_steps, actions_out, reward, terminated, stream
    "mcbs_rollout_random": (_int, [_H, _i32, _u64, _u64, _u32, _P, _P, _P, _S]),
    "mcbs_step_observe": (_int, [_H, _P, _P, _P, _INFO, _OBS, _S]),                           # batch, actions, reward, terminated, info, obs, stream
    "mcbs_observe": (_int, [_H, _OBS, _S]),                                                   # batch, obs, stream
    "mcbs_observe_masked": (_int, [_H, _OBS, _P, _S]),                                        # batch, obs, env_mask, stream
    "mcbs_action_mask": (_int, [_H, _OBS, _S]),                                               # batch, masks, stream
    "mcbs_set_mask_discrete_stride": (_int, [_H, _size]),                                     # batch, stride_bytes
    "mcbs_step_info": (_int, [_H, _INFO, _S]),                                                # batch, info, stream
    "mcbs_sample_actions": (_int, [_H, _i32, _u64, _u64, _P, _S]),                            # batch, valid, seed, step, actions_out, stream
    "mcbs_decode_attacker_actions": (_int, [_H, _P, _P, _P, _P, _S]),                         # batch, multidiscrete, discrete, actions_out, invalid_out, stream
    "mcbs_discrete_action_count": (_u64, [_H]),
    "mcbs_mask_logits": (_int, [_H, _P, _i32, _size, _f32, _S]),                              # batch, logits, dtype, row_stride, fill, stream
    "mcbs_pack_action_mask": (_int, [_H, _P, _size, _S]),                                     # batch, bits, row_words, stream
    # batch, bits, bits_row_words, logits, dtype, logits_row_stride, n_rows, fill, stream
    "mcbs_apply_packed_mask": (_int, [_H, _P, _size, _P, _i32, _size, _u64, _f32, _S]),
    "mcbs_unpack_action_mask": (_int, [_H, _P, _size, _P, _size, _u64, _S]),                  # batch, bits, bits_row_words, out, out_row_stride, n_rows, stream
    "mcbs_mask_key_words": (_u64, [_H]),
    "mcbs_store_mask_keys": (_int, [_H, _P, _size, _S]),                                      # batch, keys, row_words, stream
    # batch, keys, key_row_words, index, n_source_rows, bits, bits_row_words, n_rows, stream
    "mcbs_expand_mask_keys": (_int, [_H, _P, _size, _P, _u64, _P, _size, _u64, _S]),
    "mcbs_masked_categorical": (_int, [_H] + _CAT),                                           # batch, then _CAT
    "mcbs_masked_categorical_packed": (_int, _BITS + _CAT),                                   # _BITS, then _CAT
    "mcbs_masked_linear_categorical": (_int, [_H] + _LIN),                                    # batch, then _LIN
    "mcbs_masked_linear_categorical_packed": (_int, _BITS + _LIN),                            # _BITS, then _LIN
    # _BITS, logits, dtype, row_stride, actions, grad_log_prob, grad_entropy, grad_logits, grad_row_stride, stream
    "mcbs_masked_categorical_grad": (_int, _BITS + [_P, _i32, _size, _P, _P, _P, _P, _size, _S]),
    "mcbs_masked_linear_categorical_grad_workspace": (_size, [_H, _u64, _u32]),               # batch, n_rows, H -> bytes
    # _BITS, latent, latent_row_stride, weight, weight_row_stride, bias, H, dtype, actions, grad_log_prob, grad_entropy, grad_latent,
    # grad_latent_row_stride, grad_weight, grad_weight_row_stride, grad_bias, workspace, workspace_bytes, stream
    "mcbs_masked_linear_categorical_grad": (_int, _BITS + [_P, _size, _P, _size, _P, _u32, _i32, _P, _P, _P, _P, _size, _P, _size, _P, _P, _size, _S]),
    # batch, nvec (host), n_dims, n_rows, logits, dtype, row_stride, mode, actions, log_prob, entropy, uniforms, seed, step, row_key_base,
    # bad_actions, stream
    "mcbs_multicategorical": (_int, [_H, C.POINTER(_u32), _u32, _u64, _P, _i32, _size, _i32, _P, _P, _P, _P, _u64, _u64, _u64, _P, _S]),
    # batch, nvec (host), n_dims, n_rows, logits, dtype, row_stride, actions, grad_log_prob, grad_entropy, grad_logits, grad_row_stride, stream
    "mcbs_multicategorical_grad": (_int, [_H, C.POINTER(_u32), _u32, _u64, _P, _i32, _size, _P, _P, _P, _P, _size, _S]),
    "mcbs_gae": (_int, [_H, C.POINTER(GaeIO), _S]),                                           # batch, io, stream
    "mcbs_feature_layout_create": (_int, [_H, _P, _size, _P, _size, _NEW]),                   # batch, desc, n_desc, mask_ranges, n_mask_ranges, out
    "mcbs_feature_layout_destroy": (None, [_H]),
    "mcbs_feature_layout_width": (_u64, [_H]),
    # batch, layout, obs, bits, bits_row_words, out, dtype, out_row_stride, n_rows, out_of_range, stream
    "mcbs_encode_features": (_int, [_H, _H, _OBS, _P, _size, _P, _i32, _size, _u64, _P, _S]),
    "mcbs_obs_packing_create": (_int, [_H, _P, _size, _NEW]),                                 # batch, valid_codes, n_values, out
    "mcbs_obs_packing_destroy": (None, [_H]),
    "mcbs_obs_packing_words": (_u64, [_H]),
    "mcbs_pack_observation": (_int, [_H, _H, _OBS, _P, _size, _u64, _P, _S]),                 # batch, packing, obs, out, out_row_words, n_rows, out_of_range, stream
    # batch, packing, packed, row_words, index, n_source_rows, n_rows, out, stream
    "mcbs_unpack_observation": (_int, [_H, _H, _P, _size, _P, _u64, _u64, _OBS, _S]),
    # batch, layout, packing, packed, packed_row_words, bits, bits_row_words, index, n_source_rows, out, dtype, out_row_stride, n_rows,
    # out_of_range, stream
    "mcbs_encode_features_packed": (_int, [_H, _H, _H, _P, _size, _P, _size, _P, _u64, _P, _i32, _size, _u64, _P, _S]),
    # batch, layout, obs, n_rows, then _FL
    "mcbs_first_layer": (_int, [_H, _H, _OBS, _u64] + _FL),
    # batch, layout, packing, packed, packed_row_words, index, n_source_rows, n_rows, then _FL
    "mcbs_first_layer_packed": (_int, [_H, _H, _H, _P, _size, _P, _u64, _u64] + _FL),
    "mcbs_first_layer_grad_workspace": (_size, [_H, _H, _u64, _u32]),                         # batch, layout, n_rows, H -> bytes
    # batch, layout, obs, packing, packed, packed_row_words, index, n_source_rows, n_rows, grad_out, grad_out_row_stride, H, grad_weight_t,
    # grad_weight_row_stride, grad_bias, workspace, workspace_bytes, stream
    "mcbs_first_layer_grad": (_int, [_H, _H, _OBS, _H, _P, _size, _P, _u64, _u64, _P, _size, _u32, _P, _size, _P, _P, _size, _S]),
    "mcbs_defender_step": (_int, [_H, _P, _P, _P, _P, _DOBS, _S]),                            # batch, actions, valid, availability, evicted, obs, stream
    "mcbs_defender_observe": (_int, [_H, _DOBS, _S]),                                         # batch, obs, stream
    "mcbs_set_draw_tape": (_int, [_H, _P, _u32]),                                             # batch, tape, draws_per_step
    "mcbs_attacker_wrapper_post": (_int, [_H, _P, _f32, _i32, _S]),                           # batch, w, invalid_action_reward_modifier, max_timesteps, stream
    "mcbs_attacker_wrapper_clear": (_int, [_H, _P, _S]),                                      # batch, w, stream
    "mcbs_copy_rows_masked": (_int, [_H, _P, _P, _S]),                                        # batch, copies, env_mask, stream
    # batch, multidiscrete, discrete, decoded, info, obs, w, invalid_action_reward_modifier, max_timesteps, auto_reset, keep, fresh, stream
    "mcbs_attacker_wrapper_step": (_int, [_H, _P, _P, _P, _P, _P, _P, _f32, _i32, _i32, _P, _P, _S]),
    # batch, w, invalid_action_reward_modifier, max_timesteps, auto_reset, keep, fresh, stream
    "mcbs_attacker_wrapper_finish": (_int, [_H, _P, _f32, _i32, _i32, _P, _P, _S]),
    "mcbs_attacker_wrapper_step_launches": (_i32, [_H, _i32]),                                # batch, with_masks
    # batch, multidiscrete, discrete, decoded, info, packing, packed, packed_terminal, packed_fresh, row_words, w,
    # invalid_action_reward_modifier, max_timesteps, auto_reset, stream
    "mcbs_attacker_wrapper_step_packed": (_int, [_H, _P, _P, _P, _P, _H, _P, _P, _P, _size, _P, _f32, _i32, _i32, _S]),
    "mcbs_defender_wrapper_post": (_int, [_H, _P, _P, _S]),                                   # batch, w, cfg, stream
    "mcbs_defender_wrapper_step": (_int, [_H, _P, _P, _P, _P, _S]),                           # batch, actions, obs, w, cfg, stream
    "mcbs_defender_obs_words": (_u32, [_H]),
    "mcbs_defender_observe_packed": (_int, [_H, _P, _size, _S]),                              # batch, out, row_words, stream
    "mcbs_pack_defender_observation": (_int, [_H, _DOBS, _u64, _P, _size, _S]),               # batch, dense, n_rows, out, row_words, stream
    # batch, packed, row_words, index, n_source_rows, n_rows, out, stream
    "mcbs_unpack_defender_observation": (_int, [_H, _P, _size, _P, _u64, _u64, _DOBS, _S]),
    # batch, dense, packed, row_words, index, n_source_rows, n_rows, out, out_row_stride, dtype, bad_rows, stream
    "mcbs_encode_defender_features": (_int, [_H, _DOBS, _P, _size, _P, _u64, _u64, _P, _size, _i32, _P, _S]),
    # batch, actions, packed_out, row_words, w, cfg, stream
    "mcbs_defender_wrapper_step_packed": (_int, [_H, _P, _P, _size, _P, _P, _S]),
    "mcbs_defender_wrapper_step_packed_launches": (_i32, [_H]),
    "mcbs_two_agent_step_launches": (_i32, [_H]),
    # batch, multidiscrete, discrete, decoded, info, obs, w, invalid_action_reward_modifier, attacker_max_timesteps, defender_actions,
    # defender_obs, dw, dcfg, ep (an EpisodeBuffers block or NULL), stream
    "mcbs_two_agent_step": (_int, [_H, _P, _P, _P, _P, _P, _P, _f32, _i32, _P, _P, _P, _P, _P, _S]),
    "mcbs_two_agent_train_step_launches": (_i32, [_H]),
    # batch, multidiscrete, discrete, decoded, info, obs, w, invalid_action_reward_modifier, attacker_max_timesteps, keep, fresh,
    # defender_actions, defender_obs, dw, dcfg, tr (a TrainingBuffers block), stream
    "mcbs_two_agent_train_step": (_int, [_H, _P, _P, _P, _P, _P, _P, _f32, _i32, _P, _P, _P, _P, _P, _P, _P, _S]),
    "mcbs_two_agent_train_step_packed_launches": (_i32, [_H, _H]),                            # batch, packing
    # batch, multidiscrete, discrete, decoded, info, packing, packed, packed_terminal, packed_fresh, row_words, w,
    # invalid_action_reward_modifier, attacker_max_timesteps, defender_actions, defender_packed, defender_row_words, dw, dcfg,
    # tr (a TrainingPackedBuffers block), stream
    "mcbs_two_agent_train_step_packed": (_int, [_H, _P, _P, _P, _P, _H, _P, _P, _P, _size, _P, _f32, _i32, _P, _P, _size, _P, _P, _P, _S]),
    "mcbs_state_record_bytes": (_size, [_H]),
    "mcbs_get_state": (_int, [_H, _P, _size]),                                                # batch, host_buf, nbytes
    "mcbs_set_state": (_int, [_H, _P, _size]),                                                # batch, host_buf, nbytes
    "mcbs_batch_variant": (_int, [_H, C.POINTER(BatchVariantInfo)]),                          # batch, out
    "mcbs_step_is_lean": (_i32, [_H, _i32]),                                                  # batch, with_info
    "mcbs_topology_traits": (_int, [_P, _size, C.POINTER(_u32)]),                             # blob, nbytes, traits
    "mcbs_step_topo_traits": (_i32, [_H, _i32, C.POINTER(_u32)]),                             # batch, with_info, traits
    "mcbs_timing_enable": (_int, [_H, _i32]),                                                 # batch, on
    "mcbs_timing_read": (_int, [_H, C.POINTER(C.c_double), C.POINTER(_u64)]),                 # batch, total_ms, launches
}


STATE_HEADER_DT = np.dtype([
    ("step_count", "<u4"), ("done", "<u4"), ("truncated", "<u4"), ("episode", "<u4"),
    ("n_discovered", "<u4"), ("n_creds", "<u4"), ("last_outcome_kind", "<u4"), ("last_escalation", "<u4"),
    ("last_new_nodes", "<u4"), ("last_new_creds", "<u4"), ("last_oob", "<u4"), ("pad0", "<u4"),
    ("cum_reward", "<f8"), ("availability", "<f8")])
STATE_NODE_DT = np.dtype([
    ("discovered_props", "<u8"), ("attacked_ever", "<u4"), ("attacked_since", "<u4"),
    ("discovered", "u1"), ("installed", "u1"), ("ever_owned", "u1"), ("running", "u1"),
    ("privilege", "u1"), ("tags", "u1"), ("countdown", "u1"), ("pad", "u1"), ("pad1", "<u4", (2,))])
assert STATE_HEADER_DT.itemsize == 64 and STATE_NODE_DT.itemsize == 32


def state_record_bytes(n_nodes: int, max_creds: int) -> int:
    n = 64 + 32 * n_nodes + 2 * n_nodes + 2 * max_creds
    return (n + 15) & ~15


def split_state(buf: np.ndarray, n_envs: int, n_nodes: int, max_creds: int):
    """View a get_state buffer as (headers[E], nodes[E,N], discovery_order[E,N], credential_cache[E,C])."""
    rb = state_record_bytes(n_nodes, max_creds)
    raw = np.frombuffer(buf, dtype=np.uint8).reshape(n_envs, rb)
    hdr = raw[:, :64].copy().view(STATE_HEADER_DT).reshape(n_envs)
    nodes = raw[:, 64:64 + 32 * n_nodes].copy().view(STATE_NODE_DT).reshape(n_envs, n_nodes)
    o = 64 + 32 * n_nodes
    order = raw[:, o:o + 2 * n_nodes].copy().view("<u2").reshape(n_envs, n_nodes)
    cache = raw[:, o + 2 * n_nodes:o + 2 * n_nodes + 2 * max_creds].copy().view("<u2").reshape(n_envs, max_creds)
    return hdr, nodes, order, cache


@dataclass
class EnvSpec:
    """CyberBattleEnv constructor arguments (cyberbattle_env.py:470-485) plus batching knobs;
    lowered to mcbs_batch_cfg."""
    n_envs: int = 1
    maximum_total_credentials: int = 1000
    maximum_node_count: int = 100
    maximum_discoverable_credentials_per_action: int = 5
    # AttackerGoal (cyberbattle_env.py:227-241); None = no attacker goal
    attacker_goal: Optional[dict] = field(default_factory=lambda: dict(reward=0.0, low_availability=1.0, own_atleast=0, own_atleast_percent=1.0))
    defender_goal_eviction: bool = True
    maintain_sla: float = 0.0
    winning_reward: float = 5000.0
    losing_reward: float = 0.0
    # in-env defender: None or ("scan_and_reimage", probability, scan_capacity, scan_frequency)
    defender: Optional[tuple] = None
    auto_reset: bool = False
    max_episode_steps: int = 0
    rng_kind: int = RNG_PHILOX
    seed: int = 0
    env_id_base: int = 0
    device: int = 0

    def to_cfg(self) -> BatchCfg:
        c = BatchCfg()
        c.abi_version = ABI_VERSION
        c.n_envs = self.n_envs
        c.device = self.device
        c.maximum_node_count = self.maximum_node_count
        c.maximum_total_credentials = self.maximum_total_credentials
        c.maximum_discoverable_credentials_per_action = self.maximum_discoverable_credentials_per_action
        g = self.attacker_goal
        c.has_attacker_goal = 0 if g is None else 1
        if g is not None:
            c.goal_reward = float(g.get("reward", 0.0))
            c.goal_low_availability = float(g.get("low_availability", 1.0))
            c.goal_own_atleast = int(g.get("own_atleast", 0))
            c.goal_own_atleast_percent = float(g.get("own_atleast_percent", 1.0))
        c.defender_goal_eviction = int(bool(self.defender_goal_eviction))
        c.maintain_sla = float(self.maintain_sla)
        c.winning_reward = float(self.winning_reward)
        c.losing_reward = float(self.losing_reward)
        if self.defender is None:
            c.defender_kind = DEFENDER_NONE
            c.scan_frequency = 1
        else:
            if self.defender[0] == "external":       # learned defender acting through mcbs_defender_step
                c.defender_kind = DEFENDER_EXTERNAL
                c.scan_frequency = 1
                return self._finish(c)
            if self.defender[0] == "random_events":  # ExternalRandomEvents (defender.py:58-148): no parameters
                c.defender_kind = DEFENDER_RANDOM_EVENTS
                c.scan_frequency = 1
                return self._finish(c)
            kind, p, cap, freq = self.defender
            if kind != "scan_and_reimage":
                raise ValueError(f"unsupported in-env defender {kind!r}")
            if int(freq) <= 0 or int(cap) < 0:
                raise ValueError("scan_frequency must be positive and scan_capacity non-negative")
            c.defender_kind = DEFENDER_SCAN_AND_REIMAGE
            c.scan_probability, c.scan_capacity, c.scan_frequency = float(p), int(cap), int(freq)
        return self._finish(c)

    def _finish(self, c: BatchCfg) -> BatchCfg:
        c.auto_reset = int(bool(self.auto_reset))
        c.max_episode_steps = int(self.max_episode_steps)
        c.rng_kind = int(self.rng_kind)
        c.seed = int(self.seed) & (2 ** 64 - 1)
        c.env_id_base = int(self.env_id_base)
        return c

