"""ctypes binding of libmcbs.so (include/mcbs.h) over PyTorch-ROCm tensors.

PyTorch is plumbing here (device memory, streams); every computation is done by the HIP kernels
behind the C ABI.  There is NO CPU fallback: if the native library is missing or a call fails,
this module raises.  The CPU oracle under oracle/ is test infrastructure and is never imported
from here.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Dict, Iterable, Optional

import numpy as np

from ._abi import (CATEGORICAL_MODES, CATEGORICAL_PHILOX_DOMAIN, MCBS_LINEAR_MAX_H, PROTOTYPES, BatchCfg, BatchVariantInfo, DefenderObs,  # noqa: F401
                   EnvSpec, GaeIO, InfoBuffers, ObsBuffers, RowCopies, STATE_HEADER_DT, STATE_NODE_DT, split_state, state_record_bytes)
from .flatten import FlatTopology

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmcbs.so")

EXPORTS = list(PROTOTYPES)          # every function of include/mcbs.h: _abi.PROTOTYPES is where the C ABI is declared

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


class McbsError(RuntimeError):
    pass


def load_library(path: Optional[str] = None):
    """Load libmcbs.so; raise loudly when it is absent (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MCBS_LIBRARY") or LIB_PATH      # MCBS_LIBRARY: developer override (e.g. the -DMCBS_DIAG build)
    if not os.path.exists(p):
        raise NativeLibraryMissing(
            f"{p} not found: the HIP extension has not been built. Build it with `make -C marlon_amd/csrc` "
            f"(hipcc, gfx950). There is no CPU fallback for the step engine.")
    # torch first: it ships its own HIP runtime (torch/lib/libamdhip64.so), and the first copy a process maps is the one every later
    # library with that soname binds to.  Loaded before torch, libmcbs.so pulled in /opt/rocm's runtime and torch then ran on a runtime it
    # was not built against ("no ROCm-capable device is detected" from the first allocation; build() followed by smoke() in one process).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise NativeLibraryMissing(f"{p} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int, what: str) -> None:
    if rc != 0:
        raise McbsError(f"{what} failed ({rc}): {lib.mcbs_last_error().decode(errors='replace')}")


def _ptr(x):
    """The device pointer of an optional tensor (None: NULL)."""
    return x.data_ptr() if x is not None else None


_U64 = 2 ** 64 - 1


def _u64(v) -> int:
    """A seed, step or row key as the uint64_t the library takes (negative and oversized Python ints wrap)."""
    return int(v) & _U64


def _describe(x) -> str:
    """What a refused argument was, for the message: a tensor's dtype, shape, strides and device, else its type."""
    if hasattr(x, "stride") and hasattr(x, "device"):
        return f"{x.dtype} {list(x.shape)} with strides {list(x.stride())} on {x.device}"
    return type(x).__name__


def _row_stride(x, rows: int) -> int:
    """The row stride in elements handed to the library for x, a 2-D tensor whose row count `rows` the caller has already checked
    (x None: 0).  torch reports an arbitrary stride(0) for a dimension of size 1, so a one-row tensor's is raised to its width: the C
    side refuses a stride below the columns it uses."""
    if x is None:
        return 0
    return x.stride(0) if rows > 1 else max(x.stride(0), x.shape[1])


# BatchEngine._bound: where the per-call values go in a bound call's argument list
_ACTIONS, _ACTIONS2, _EPISODE, _STREAM = "<actions>", "<second actions>", "<episode block>", "<stream>"


def _attacker_actions(discrete: bool):
    """The attacker entry points' (MultiDiscrete rows, Discrete indices) pointer pair: the call's actions in the one, NULL in the other."""
    return (None, _ACTIONS) if discrete else (_ACTIONS, None)


def topology_traits(topo: FlatTopology) -> int:
    """The MCBS_TOPO_* bits (_abi.TOPO_*) the native library derives from a topology's blob; computed on the host, no GPU needed."""
    lib = load_library()
    blob = np.frombuffer(topo.blob, dtype=np.uint8)
    t = C.c_uint32()
    _check(lib, lib.mcbs_topology_traits(blob.ctypes.data, blob.size, C.byref(t)), "mcbs_topology_traits")
    return int(t.value)


def obs_field_shapes(topo: FlatTopology, spec: EnvSpec) -> Dict[str, tuple]:
    N, Cm, K = spec.maximum_node_count, spec.maximum_total_credentials, spec.maximum_discoverable_credentials_per_action
    L, R, P = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports)
    return {
        "scalars": ((7,), "int32"), "leaked_credentials": ((K, 4), "int32"), "credential_cache_matrix": ((Cm, 2), "int32"),
        "discovered_nodes_properties": ((N, len(topo.properties)), "int32"), "nodes_privilegelevel": ((N,), "int32"),
        "mask_local": ((N, L), "int8"), "mask_remote": ((N, N, R), "int8"), "mask_connect": ((N, N, P, Cm), "int8"),
        "mask_discrete": ((N * N * P * Cm + N * L + N * N * R,), "int8"),
    }


class FeatureLayoutHandle:
    """A `features.FeatureLayout` handed to the library (mcbs_feature_layout_create): descriptors uploaded once, freed with the object."""

    def __init__(self, lib, ptr, layout):
        self.lib, self.ptr, self.layout = lib, ptr, layout
        self.width = int(lib.mcbs_feature_layout_width(ptr))
        self.has_masks = layout.mask_columns > 0

    def close(self) -> None:
        if getattr(self, "ptr", None):
            self.lib.mcbs_feature_layout_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObservationPackingHandle:
    """A `features.ObservationPacking` handed to the library (mcbs_obs_packing_create): descriptors uploaded once, freed with the object."""

    def __init__(self, lib, ptr, packing):
        self.lib, self.ptr, self.packing = lib, ptr, packing
        self.words = int(lib.mcbs_obs_packing_words(ptr))

    def close(self) -> None:
        if getattr(self, "ptr", None):
            self.lib.mcbs_obs_packing_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# what BatchEngine.masked_categorical returns: actions int64 [n], log_prob float32 [n], entropy float32 [n], n_allowed int32 [n]
MaskedCategorical = collections.namedtuple("MaskedCategorical", ["actions", "log_prob", "entropy", "n_allowed"])

_MASKED_EVALUATE = None


def _masked_evaluate_function(torch):
    """The torch.autograd.Function behind BatchEngine.masked_evaluate (made on first use: this module does not import torch at load)."""
    global _MASKED_EVALUATE
    if _MASKED_EVALUATE is not None:
        return _MASKED_EVALUATE

    class MaskedEvaluate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, eng, bits, actions, bad_actions):
            r = eng.masked_categorical(logits, bits=bits, mode="evaluate", actions=actions, bad_actions=bad_actions)
            ctx.eng = eng
            ctx.save_for_backward(logits, bits, actions)
            ctx.mark_non_differentiable(r.n_allowed)
            ctx.set_materialize_grads(False)             # an output the loss does not use arrives as None, not as zeros
            return r.log_prob, r.entropy, r.n_allowed

        @staticmethod
        def backward(ctx, g_lp, g_ent, _g_k):
            logits, bits, actions = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None, None, None, None
            grad = ctx.eng.masked_categorical_grad(logits, bits, actions,
                                                   None if g_lp is None else g_lp.float().contiguous(),
                                                   None if g_ent is None else g_ent.float().contiguous())
            return grad, None, None, None, None

    _MASKED_EVALUATE = MaskedEvaluate
    return MaskedEvaluate


# what BatchEngine.masked_linear_categorical_grad returns: float32 [n, H], [A, H], [A]; None for a gradient that was not asked for
MaskedLinearGrad = collections.namedtuple("MaskedLinearGrad", ["grad_latent", "grad_weight", "grad_bias"])

_MASKED_LINEAR_EVALUATE = None


def _masked_linear_evaluate_function(torch):
    """The torch.autograd.Function behind BatchEngine.masked_linear_evaluate (made on first use, like _masked_evaluate_function)."""
    global _MASKED_LINEAR_EVALUATE
    if _MASKED_LINEAR_EVALUATE is not None:
        return _MASKED_LINEAR_EVALUATE

    class MaskedLinearEvaluate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, latent, weight, bias, eng, bits, actions, bad_actions):
            r = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode="evaluate", actions=actions, bad_actions=bad_actions)
            ctx.eng = eng
            ctx.has_bias = bias is not None
            ctx.save_for_backward(*((latent, weight, bits, actions) + ((bias,) if bias is not None else ())))
            ctx.mark_non_differentiable(r.n_allowed)
            ctx.set_materialize_grads(False)             # an output the loss does not use arrives as None, not as zeros
            return r.log_prob, r.entropy, r.n_allowed

        @staticmethod
        def backward(ctx, g_lp, g_ent, _g_k):
            latent, weight, bits, actions = ctx.saved_tensors[:4]
            bias = ctx.saved_tensors[4] if ctx.has_bias else None
            want = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
            if not any(want):
                return (None,) * 7
            g = ctx.eng.masked_linear_categorical_grad(latent, weight, bias, bits, actions,
                                                       None if g_lp is None else g_lp.float().contiguous(),
                                                       None if g_ent is None else g_ent.float().contiguous(), want=want)
            return tuple(None if x is None else x.to(latent.dtype) for x in g) + (None,) * 4

    _MASKED_LINEAR_EVALUATE = MaskedLinearEvaluate
    return MaskedLinearEvaluate


# what BatchEngine.multicategorical returns: actions int64 [n, D], log_prob float32 [n], entropy float32 [n]
MultiCategorical = collections.namedtuple("MultiCategorical", ["actions", "log_prob", "entropy"])

_MULTI_EVALUATE = None


def _multicategorical_evaluate_function(torch):
    """The torch.autograd.Function behind BatchEngine.multicategorical_evaluate (made on first use, like _masked_evaluate_function)."""
    global _MULTI_EVALUATE
    if _MULTI_EVALUATE is not None:
        return _MULTI_EVALUATE

    class MultiCategoricalEvaluate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, eng, nvec, actions, bad_actions):
            r = eng.multicategorical(logits, nvec, mode="evaluate", actions=actions, bad_actions=bad_actions)
            ctx.eng, ctx.nvec = eng, nvec
            ctx.save_for_backward(logits, actions)
            ctx.set_materialize_grads(False)             # an output the loss does not use arrives as None, not as zeros
            return r.log_prob, r.entropy

        @staticmethod
        def backward(ctx, g_lp, g_ent):
            logits, actions = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None, None, None, None
            grad = ctx.eng.multicategorical_grad(logits, ctx.nvec, actions,
                                                 None if g_lp is None else g_lp.float().contiguous(),
                                                 None if g_ent is None else g_ent.float().contiguous())
            return grad, None, None, None, None

    _MULTI_EVALUATE = MultiCategoricalEvaluate
    return MultiCategoricalEvaluate


# what BatchEngine.first_layer_grad returns: float32 [F, H] and [H]; None for a gradient that was not asked for
FirstLayerGrad = collections.namedtuple("FirstLayerGrad", ["grad_weight_t", "grad_bias"])

_FIRST_LAYER_EVALUATE = None


def _first_layer_evaluate_function(torch):
    """The torch.autograd.Function behind BatchEngine.first_layer_evaluate (made on first use, like _masked_evaluate_function)."""
    global _FIRST_LAYER_EVALUATE
    if _FIRST_LAYER_EVALUATE is not None:
        return _FIRST_LAYER_EVALUATE

    class FirstLayerEvaluate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, weight, bias, eng, handle, source, dtype, out_of_range, weight_t):
            if weight_t is None:
                weight_t = weight.detach().t().contiguous()          # torch's [H, F] -> the [F, H] the kernel reads (Chain-10 at H = 64: 259 KB)
            ctx.eng, ctx.handle, ctx.source = eng, handle, source    # (integer inputs: no gradient, nothing for autograd to track)
            ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype)
            return eng.first_layer(handle, weight_t, None if bias is None else bias.detach(), dtype=dtype, out_of_range=out_of_range, **source)

        @staticmethod
        def backward(ctx, g):
            want = (ctx.needs_input_grad[0], ctx.dtypes[1] is not None and ctx.needs_input_grad[1])
            if g is None or not any(want):
                return (None,) * 8
            r = ctx.eng.first_layer_grad(ctx.handle, g.float().contiguous(), want=want, **ctx.source)
            return (None if r.grad_weight_t is None else r.grad_weight_t.t().to(ctx.dtypes[0]),
                    None if r.grad_bias is None else r.grad_bias.to(ctx.dtypes[1])) + (None,) * 6

    _FIRST_LAYER_EVALUATE = FirstLayerEvaluate
    return FirstLayerEvaluate


FEATURE_FIELDS = ("scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel")


class BatchEngine:
    """n_envs CyberBattleSim environments sharing one topology, advanced on one MI355X."""

    def __init__(self, topo: FlatTopology, spec: EnvSpec, device: Optional[str] = None):
        import torch

        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise McbsError("no HIP device visible to PyTorch: the step engine needs a GPU (there is no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{spec.device}")
        spec.device = self.device.index or 0
        self.topo, self.spec = topo, spec
        self.E = spec.n_envs
        blob = np.frombuffer(topo.blob, dtype=np.uint8)
        self._topo_h = C.c_void_p()
        _check(self.lib, self.lib.mcbs_topology_create(blob.ctypes.data, blob.size, spec.device, C.byref(self._topo_h)), "mcbs_topology_create")
        self._cfg = spec.to_cfg()
        self._h = C.c_void_p()
        rc = self.lib.mcbs_batch_create(self._topo_h, C.byref(self._cfg), C.byref(self._h))
        if rc != 0:
            msg = self.lib.mcbs_last_error().decode(errors="replace")
            self.lib.mcbs_topology_destroy(self._topo_h)
            self._topo_h = None
            raise (ValueError if rc == -1 else McbsError)(f"mcbs_batch_create failed ({rc}): {msg}")
        self._shapes = obs_field_shapes(topo, spec)
        self.mask_discrete_stride = 0
        self._tape = None
        self._raw_stream = None
        f32, u8, f64, i32 = torch.float32, torch.uint8, torch.float64, torch.int32
        dev = self.device
        self.reward = torch.zeros(self.E, dtype=f32, device=dev)
        self.terminated = torch.zeros(self.E, dtype=u8, device=dev)
        self.info = dict(network_availability=torch.zeros(self.E, dtype=f64, device=dev),
                         step_count=torch.zeros(self.E, dtype=i32, device=dev),
                         truncated=torch.zeros(self.E, dtype=u8, device=dev),
                         out_of_bound=torch.zeros(self.E, dtype=u8, device=dev),
                         raw_reward=torch.zeros(self.E, dtype=f32, device=dev))
        self._info_struct = InfoBuffers(**{k: v.data_ptr() for k, v in self.info.items()})
        self._feature_rows = {k: int(np.prod(self._shapes[k][0])) for k in FEATURE_FIELDS}        # int32 values per row of each field
        # fixed at creation, and wanted by the checks of nearly every call below: asked of the library once
        self._A, self._Wk = int(self.lib.mcbs_discrete_action_count(self._h)), int(self.lib.mcbs_mask_key_words(self._h))
        self._nvec_blocks = {}                             # multicategorical: nvec tuple -> (host uint32 array, D, A)
        self._feature_dtypes = {torch.float32: (0, 4), torch.bfloat16: (1, 2), torch.float16: (2, 2)}  # MCBS_FEATURES_* code, item size

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.torch.cuda.synchronize(self.device)
            self.lib.mcbs_batch_destroy(self._h)
            self._h = None
            self._A = self._Wk = 0                  # what the library answers for a null batch
        if getattr(self, "_topo_h", None):
            self.lib.mcbs_topology_destroy(self._topo_h)
            self._topo_h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers --
    def _stream(self) -> int:
        """The raw handle of torch's current stream on this engine's device (queried per call: the caller may switch streams)."""
        raw = self._raw_stream
        if raw is None:
            # torch's C binding answers in ~0.2 us; the Python-level current_stream() builds a Stream object first (~1.5 us of a ~10 us call)
            get = getattr(self.torch._C, "_cuda_getCurrentRawStream", None)
            idx = self.device.index if self.device.index is not None else self.torch.cuda.current_device()
            raw = self._raw_stream = (lambda: get(idx)) if get is not None else (lambda: self.torch.cuda.current_stream(self.device).cuda_stream)
        return raw()

    def alloc_obs(self, fields: Optional[Iterable[str]] = None) -> dict:
        t = self.torch
        out = {}
        for f in (fields or [k for k in self._shapes if k != "mask_discrete"]):
            shape, dt = self._shapes[f]
            if f == "mask_discrete" and self.mask_discrete_stride:
                shape = (self.mask_discrete_stride,)          # padded rows (set_mask_discrete_stride): [:, :discrete_action_count()] is the mask
            out[f] = t.zeros((self.E,) + shape, dtype=getattr(t, dt), device=self.device)
        return out

    def set_mask_discrete_stride(self, stride_bytes: int) -> None:
        """Rows of `mask_discrete` buffers handed to this engine are `stride_bytes` apart (0: dense).  A multiple of 128 puts every env's
        mask on cache lines of its own (mcbs_set_mask_discrete_stride); alloc_obs then allocates padded rows."""
        _check(self.lib, self.lib.mcbs_set_mask_discrete_stride(self._h, int(stride_bytes)), "mcbs_set_mask_discrete_stride")
        self.mask_discrete_stride = int(stride_bytes)

    @staticmethod
    def _obs_struct(obs: dict) -> ObsBuffers:
        return ObsBuffers(**{k: v.data_ptr() for k, v in obs.items()})

    def _actions(self, actions):
        t = self.torch
        a = actions if isinstance(actions, t.Tensor) else t.as_tensor(np.asarray(actions), device=self.device)
        a = a.to(device=self.device, dtype=t.int32).contiguous()
        if tuple(a.shape) != (self.E, 5):
            raise ValueError(f"actions must have shape ({self.E}, 5), got {tuple(a.shape)}")
        return a

    # the checks on tensor arguments every call below shares: each raises ValueError naming the argument, and returns the tensor
    def _arr(self, x, dtype, shape, what: str):
        """x: a contiguous device tensor of exactly this dtype and shape."""
        if not isinstance(x, self.torch.Tensor) or x.dtype != dtype or x.device != self.device or tuple(x.shape) != shape or not x.is_contiguous():
            raise ValueError(f"{what} must be a contiguous device {dtype} tensor {list(shape)}, got {_describe(x)}")
        return x

    def _rows(self, x, dtypes, what: str, n=None, min_cols: int = 0):
        """x: a device tensor [n, >= min_cols] (n None: any count) of one of `dtypes` with unit inner stride; the rows may lie further
        apart.  The C side sees only the row stride: a view narrower than min_cols would have its rows read or written past their end."""
        if (not isinstance(x, self.torch.Tensor) or x.dtype not in dtypes or x.dim() != 2 or (n is not None and x.shape[0] != n)
                or x.stride(1) != 1 or x.device != self.device or x.shape[1] < min_cols):
            names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
            raise ValueError(f"{what} must be a device {names} tensor [{'n' if n is None else n}, >= {min_cols}] with contiguous rows, "
                             f"got {_describe(x)}")
        return x

    def _counter(self, x, what: str):
        """x: the device int32 tensor of one element a call adds a count to (bad_actions, out_of_range)."""
        if not isinstance(x, self.torch.Tensor) or x.dtype != self.torch.int32 or x.numel() != 1 or x.device != self.device:
            raise ValueError(f"{what} must be a device int32 tensor of one element, got {_describe(x)}")
        return x

    def _dtype_code(self, x) -> int:
        """MCBS_LOGITS_F32 / MCBS_LOGITS_BF16 of a tensor already checked to be one of the two."""
        return 0 if x.dtype == self.torch.float32 else 1

    def _logits(self, x, n, A: int):
        """x: float32 or bfloat16 logits [n, >= A] (n None: any count) -> (pointer, dtype code, row stride): the three arguments every
        entry point takes for them (a call with a uniform law passes None, 0, 0 for logits=None)."""
        self._rows(x, (self.torch.float32, self.torch.bfloat16), "logits", n, A)
        return x.data_ptr(), self._dtype_code(x), _row_stride(x, x.shape[0] if n is None else n)

    # -- the C ABI --
    def reset(self, env_mask=None) -> None:
        ptr = None
        if env_mask is not None:
            env_mask = env_mask.to(device=self.device, dtype=self.torch.uint8).contiguous()
            ptr = env_mask.data_ptr()
        _check(self.lib, self.lib.mcbs_reset(self._h, ptr, self._stream()), "mcbs_reset")

    def rewind(self) -> None:
        """Every env back to the state right after creation (episode counters 0): a recorded trajectory replays exactly, defender draws included."""
        _check(self.lib, self.lib.mcbs_rewind(self._h, self._stream()), "mcbs_rewind")

    def set_draw_tape(self, tape) -> None:
        t = self.torch
        if tape is None:
            self._tape = None
            _check(self.lib, self.lib.mcbs_set_draw_tape(self._h, None, 0), "mcbs_set_draw_tape")
            return
        tape = tape if isinstance(tape, t.Tensor) else t.as_tensor(np.asarray(tape, dtype=np.float64))
        self._tape = tape.to(device=self.device, dtype=t.float64).reshape(self.E, -1).contiguous()
        _check(self.lib, self.lib.mcbs_set_draw_tape(self._h, self._tape.data_ptr(), self._tape.shape[1]), "mcbs_set_draw_tape")

    def step(self, actions, with_info: bool = True):
        """One CyberBattleEnv.step for every env (observation excluded).  Returns (reward, terminated) device tensors,
        overwritten by the next call; self.info holds StepInfo tensors when with_info."""
        a = self._actions(actions)
        _check(self.lib, self.lib.mcbs_step(self._h, a.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                                            C.byref(self._info_struct) if with_info else None, self._stream()), "mcbs_step")
        return self.reward, self.terminated

    def step_many(self, actions, rewards=None, terminated=None):
        """K consecutive steps in one launch: actions [K, E, 5] int32 on the device (a recorded / scripted / pre-sampled sequence).
        Returns (rewards [K, E] float32, terminated [K, E] uint8); same results as K calls of step()."""
        t = self.torch
        a = actions if (isinstance(actions, t.Tensor) and actions.dtype == t.int32 and actions.is_contiguous() and
                        actions.device == self.device) else t.as_tensor(actions, dtype=t.int32, device=self.device).contiguous()
        if a.dim() != 3 or a.shape[1] != self.E or a.shape[2] != 5:
            raise ValueError(f"actions must be [K, {self.E}, 5]")
        K = a.shape[0]
        rewards = t.empty((K, self.E), dtype=t.float32, device=self.device) if rewards is None else rewards
        terminated = t.empty((K, self.E), dtype=t.uint8, device=self.device) if terminated is None else terminated
        _check(self.lib, self.lib.mcbs_step_many(self._h, a.data_ptr(), rewards.data_ptr(), terminated.data_ptr(), K, self._stream()),
               "mcbs_step_many")
        return rewards, terminated

    def rollout_random(self, n_steps: int, valid: bool = True, seed: int = 0, first_step: int = 0, record_actions: bool = False):
        """Random agents for n_steps steps in one launch (actions sampled inside the kernel, the distribution of sample_valid_action
        or uniform).  Returns (rewards [K, E], terminated [K, E], actions [K, E, 5] or None)."""
        t = self.torch
        rewards = t.empty((n_steps, self.E), dtype=t.float32, device=self.device)
        terminated = t.empty((n_steps, self.E), dtype=t.uint8, device=self.device)
        actions = t.empty((n_steps, self.E, 5), dtype=t.int32, device=self.device) if record_actions else None
        _check(self.lib, self.lib.mcbs_rollout_random(self._h, int(bool(valid)), _u64(seed), int(first_step), int(n_steps),
                                                      None if actions is None else actions.data_ptr(), rewards.data_ptr(),
                                                      terminated.data_ptr(), self._stream()), "mcbs_rollout_random")
        return rewards, terminated, actions

    def wrapper_post(self, bufs, modifier: float, max_timesteps: int) -> None:
        """AttackerEnvWrapper.step's bookkeeping for every env in one launch; `bufs` is a _abi.WrapperBuffers of device pointers."""
        _check(self.lib, self.lib.mcbs_attacker_wrapper_post(self._h, C.byref(bufs), float(modifier), int(max_timesteps), self._stream()),
               "mcbs_attacker_wrapper_post")

    def defender_wrapper_post(self, bufs, cfg) -> None:
        """DefenderEnvWrapper.step's reward shaping for every env in one launch (_abi.DefenderWrapperBuffers / DefenderWrapperCfg)."""
        _check(self.lib, self.lib.mcbs_defender_wrapper_post(self._h, C.byref(bufs), C.byref(cfg), self._stream()), "mcbs_defender_wrapper_post")

    def copy_rows_masked(self, pairs, env_mask) -> None:
        """dst[e] = src[e] for the envs whose byte in env_mask (uint8 [E], device) is set, for up to eight (src, dst) pairs of
        contiguous [E, ...] tensors in one launch."""
        if not 0 < len(pairs) <= 8:
            raise ValueError("copy_rows_masked takes one to eight (src, dst) pairs")
        rc = RowCopies()
        rc.n = len(pairs)
        for i, (src, dst) in enumerate(pairs):
            if src.shape != dst.shape or src.dtype != dst.dtype or not (src.is_contiguous() and dst.is_contiguous()) or src.shape[0] != self.E:
                raise ValueError("copy_rows_masked needs contiguous [E, ...] tensors of the same shape and dtype")
            rc.src[i], rc.dst[i], rc.row_bytes[i] = src.data_ptr(), dst.data_ptr(), src[0].numel() * src.element_size()
        _check(self.lib, self.lib.mcbs_copy_rows_masked(self._h, C.byref(rc), env_mask.data_ptr(), self._stream()), "mcbs_copy_rows_masked")

    def _row_copies(self, pairs, one_row_src: bool):
        if len(pairs) > 8:
            raise ValueError("at most eight (src, dst) pairs per list")
        rc = RowCopies()
        rc.n = len(pairs)
        for i, (src, dst) in enumerate(pairs):
            rows = 1 if one_row_src else self.E
            if src.shape[1:] != dst.shape[1:] or src.dtype != dst.dtype or not (src.is_contiguous() and dst.is_contiguous()) or \
                    src.shape[0] != rows or dst.shape[0] != self.E:
                raise ValueError("row copies need contiguous tensors of the same row shape and dtype ([E, ...]; reset rows: [1, ...])")
            rc.src[i], rc.dst[i], rc.row_bytes[i] = src.data_ptr(), dst.data_ptr(), dst[0].numel() * dst.element_size()
        return rc

    def _bound(self, name: str, *args, keep=()):
        """callable(p), or callable(p, q, ep=None) where args hold _ACTIONS2: the library function `name` on this batch with every argument but
        the per-call ones bound ONCE — the argument blocks' references and conversions are most of what a per-step call costs on the host next to the launch itself.
        args: what follows the batch handle, in the prototype's order: numbers and None as they are, a tensor as its device pointer, a
        ctypes block as a reference to it; and, by position, the per-call values: _ACTIONS <- p, _ACTIONS2 <- q (actions pointers),
        _EPISODE <- a reference to ep (an _abi.EpisodeBuffers the caller keeps alive) or NULL, _STREAM <- torch's current stream, queried
        per call.  The batch handle is read per call too (None once the engine is closed: the library refuses it); a failure raises
        through _check under the entry point's name.  The closure keeps alive every tensor and block it points into, and `keep`."""
        fn, eng, lib, stream = getattr(self.lib, name), self, self.lib, self._stream
        Tensor, blocks = self.torch.Tensor, (C.Structure, C.Array)
        argv = [None] + [x.data_ptr() if isinstance(x, Tensor) else C.byref(x) if isinstance(x, blocks) else x for x in args]
        ip, iq, ie, ist = (argv.index(m) if m in argv else None for m in (_ACTIONS, _ACTIONS2, _EPISODE, _STREAM))
        if ie is not None:
            argv[ie] = None

        # one pointer or two: a missing or a surplus actions pointer is a TypeError on the host, as is an episode block handed to an entry
        # point that has no _EPISODE slot (ie is None).  The two bodies end alike; a shared tail would cost every step a Python call.
        if iq is None:
            if ie is not None:
                raise ValueError(f"{name}: an episode block without second actions")

            def call(p: int, *, _alive=(args, keep)) -> None:
                a = argv.copy()
                a[0], a[ip], a[ist] = eng._h, p, stream()
                rc = fn(*a)
                if rc:
                    _check(lib, rc, name)
        else:
            def call(p: int, q: int, ep=None, *, _alive=(args, keep)) -> None:
                a = argv.copy()
                a[0], a[ip], a[iq], a[ist] = eng._h, p, q, stream()
                if ep is not None:
                    a[ie] = C.byref(ep)
                rc = fn(*a)
                if rc:
                    _check(lib, rc, name)
        return call

    def wrapper_step_call(self, discrete: bool, decoded, obs_struct, bufs, modifier: float, max_timesteps: int, auto_reset: bool, keep, fresh):
        """callable(actions_ptr): mcbs_attacker_wrapper_step — decode, environment step + observation, bookkeeping / auto-reset — with every
        argument but the actions bound once (_bound).  `decoded`: int32 [E, 5]; `obs_struct`: obs_struct(obs); `bufs` / `keep` / `fresh`:
        argument blocks built once (WrapperBuffers, row_copies())."""
        return self._bound("mcbs_attacker_wrapper_step", *_attacker_actions(discrete), decoded, self._info_struct, obs_struct, bufs, float(modifier),
                           int(max_timesteps), int(bool(auto_reset)), keep, fresh, _STREAM)

    def wrapper_step_packed_call(self, discrete: bool, decoded, packing: "ObservationPackingHandle", packed, packed_terminal, packed_fresh, bufs,
                                 modifier: float, max_timesteps: int, auto_reset: bool):
        """callable(actions_ptr): mcbs_attacker_wrapper_step_packed — the one-launch wrapper step that writes the packed observation row
        instead of the five int32 fields — bound once like wrapper_step_call.  packed / packed_terminal: device int32 [E, >= W_obs] with
        contiguous rows and one row stride (packed_terminal may be None without auto_reset); packed_fresh: int32 [>= W_obs] or
        [1, >= W_obs], the packed row of a freshly reset env.  The library refuses a batch whose wrapper step is not one launch."""
        t = self.torch
        self._packed_obs_rows(packed, packing, "packed", self.E)
        stride = _row_stride(packed, self.E)
        if packed_terminal is not None:
            self._packed_obs_rows(packed_terminal, packing, "packed_terminal", self.E)
            if _row_stride(packed_terminal, self.E) != stride:
                raise ValueError("packed and packed_terminal must have the same row stride")
        if packed_fresh is not None:
            if packed_fresh.dtype != t.int32 or packed_fresh.device != self.device or not packed_fresh.is_contiguous() or packed_fresh.numel() < packing.words:
                raise ValueError(f"packed_fresh must be a contiguous device int32 tensor of at least {packing.words} words, got {_describe(packed_fresh)}")
        return self._bound("mcbs_attacker_wrapper_step_packed", *_attacker_actions(discrete), decoded, self._info_struct, packing.ptr, packed,
                           packed_terminal, packed_fresh, stride, bufs, float(modifier), int(max_timesteps), int(bool(auto_reset)), _STREAM,
                           keep=(packing,))

    def defender_wrapper_step_call(self, obs_struct, bufs, cfg):
        """callable(actions_ptr): mcbs_defender_wrapper_step — the defender's turn + the wrapper's reward shaping in one launch, then the
        observation — with the argument blocks bound once.  `obs_struct`: a DefenderObs block (or None)."""
        return self._bound("mcbs_defender_wrapper_step", _ACTIONS, obs_struct, bufs, cfg, _STREAM)

    def two_agent_step_launches(self) -> int:
        """1 when mcbs_two_agent_step serves this batch (both wrappers' steps and the episode bookkeeping in one launch), else 0."""
        return int(self.lib.mcbs_two_agent_step_launches(self._h))

    def two_agent_step_call(self, discrete: bool, decoded, obs_struct, bufs, modifier: float, max_timesteps: int, defender_obs_struct, defender_bufs,
                            defender_cfg):
        """callable(attacker_actions_ptr, defender_actions_ptr, episode_block or None): mcbs_two_agent_step with every argument block but
        the episode's bound once, like wrapper_step_call / defender_wrapper_step_call.  `episode_block`: an _abi.EpisodeBuffers the caller
        keeps alive (its two reward rows move from turn to turn)."""
        return self._bound("mcbs_two_agent_step", *_attacker_actions(discrete), decoded, self._info_struct, obs_struct, bufs, float(modifier),
                           int(max_timesteps), _ACTIONS2, defender_obs_struct, defender_bufs, defender_cfg, _EPISODE, _STREAM)

    def two_agent_train_step_launches(self) -> int:
        """1 when mcbs_two_agent_train_step serves this batch (the training turn: both wrappers' steps, both auto-resets and the
        reset_request hand-shake in one launch), else 0."""
        return int(self.lib.mcbs_two_agent_train_step_launches(self._h))

    def two_agent_train_step_call(self, discrete: bool, decoded, obs_struct, bufs, modifier: float, max_timesteps: int, keep, fresh,
                                  defender_obs_struct, defender_bufs, defender_cfg, training_block):
        """callable(attacker_actions_ptr, defender_actions_ptr): mcbs_two_agent_train_step with every argument block bound once, like
        two_agent_step_call.  keep / fresh: row_copies() blocks that pair every observation field with its terminal array and its reset
        row; training_block: an _abi.TrainingBuffers whose arrays the caller keeps alive."""
        return self._bound("mcbs_two_agent_train_step", *_attacker_actions(discrete), decoded, self._info_struct, obs_struct, bufs, float(modifier),
                           int(max_timesteps), keep, fresh, _ACTIONS2, defender_obs_struct, defender_bufs, defender_cfg, training_block, _STREAM)

    def two_agent_train_step_packed_launches(self, packing: "ObservationPackingHandle") -> int:
        """1 when mcbs_two_agent_train_step_packed serves this batch with this packing (the training turn with both observations written
        as packed rows by its one launch), else 0."""
        return int(self.lib.mcbs_two_agent_train_step_packed_launches(self._h, packing.ptr))

    def two_agent_train_step_packed_call(self, discrete: bool, decoded, packing: "ObservationPackingHandle", packed, packed_terminal, packed_fresh,
                                         bufs, modifier: float, max_timesteps: int, defender_packed, defender_bufs, defender_cfg, training_block):
        """callable(attacker_actions_ptr, defender_actions_ptr): mcbs_two_agent_train_step_packed with every argument block bound once, like
        two_agent_train_step_call.  packed / packed_terminal / packed_fresh: the attacker's rows as wrapper_step_packed_call takes them;
        defender_packed: device int32 [E, >= W_def] with contiguous rows, the defender's live rows — the terminal rows named by
        training_block (an _abi.TrainingPackedBuffers whose arrays the caller keeps alive) have the same row stride."""
        t = self.torch
        for x, what in ((packed, "packed"), (packed_terminal, "packed_terminal")):
            self._packed_obs_rows(x, packing, what, self.E)
        stride = _row_stride(packed, self.E)
        if _row_stride(packed_terminal, self.E) != stride:
            raise ValueError("packed and packed_terminal must have the same row stride")
        if packed_fresh.dtype != t.int32 or packed_fresh.device != self.device or not packed_fresh.is_contiguous() or packed_fresh.numel() < packing.words:
            raise ValueError(f"packed_fresh must be a contiguous device int32 tensor of at least {packing.words} words, got {_describe(packed_fresh)}")
        self._defender_packed_rows(defender_packed, "defender_packed", self.E)
        return self._bound("mcbs_two_agent_train_step_packed", *_attacker_actions(discrete), decoded, self._info_struct, packing.ptr, packed,
                           packed_terminal, packed_fresh, stride, bufs, float(modifier), int(max_timesteps), _ACTIONS2, defender_packed,
                           _row_stride(defender_packed, self.E), defender_bufs, defender_cfg, training_block, _STREAM, keep=(packing,))

    def wrapper_step_launches(self, with_masks: bool) -> int:
        """Kernel launches per mcbs_attacker_wrapper_step of this batch (1: the whole wrapper step is one launch; 3 otherwise)."""
        return int(self.lib.mcbs_attacker_wrapper_step_launches(self._h, int(bool(with_masks))))

    def obs_struct(self, obs: dict):
        """Argument block (_abi.ObsBuffers) for wrapper_step_call and the two-agent calls, built once for a set of persistent observation tensors."""
        return self._obs_struct(obs)

    def row_copies(self, pairs, one_row_src: bool = False):
        """Argument block (_abi.RowCopies) for wrapper_step_call's keep / fresh lists, built once and reused across steps."""
        return self._row_copies(list(pairs), one_row_src)

    def wrapper_clear(self, bufs) -> None:
        _check(self.lib, self.lib.mcbs_attacker_wrapper_clear(self._h, C.byref(bufs), self._stream()), "mcbs_attacker_wrapper_clear")

    def step_observe(self, actions, obs: dict):
        a = self._actions(actions)
        b = self._obs_struct(obs)
        _check(self.lib, self.lib.mcbs_step_observe(self._h, a.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                                                    C.byref(self._info_struct), C.byref(b), self._stream()), "mcbs_step_observe")
        return self.reward, self.terminated

    def observe(self, obs: dict, env_mask=None) -> dict:
        b = self._obs_struct(obs)
        if env_mask is None:
            _check(self.lib, self.lib.mcbs_observe(self._h, C.byref(b), self._stream()), "mcbs_observe")
        else:
            env_mask = env_mask.to(device=self.device, dtype=self.torch.uint8).contiguous()
            _check(self.lib, self.lib.mcbs_observe_masked(self._h, C.byref(b), env_mask.data_ptr(), self._stream()), "mcbs_observe_masked")
        return obs

    def action_mask(self, masks: dict) -> dict:
        """compute_action_mask for every env: fills the mask_* tensors given (current state, never blank)."""
        b = self._obs_struct({k: v for k, v in masks.items() if k.startswith("mask_")})
        _check(self.lib, self.lib.mcbs_action_mask(self._h, C.byref(b), self._stream()), "mcbs_action_mask")
        return masks

    def step_info(self) -> dict:
        _check(self.lib, self.lib.mcbs_step_info(self._h, C.byref(self._info_struct), self._stream()), "mcbs_step_info")
        return self.info

    def sample_actions(self, valid: bool, seed: int, step: int, out=None):
        t = self.torch
        if out is None:
            out = t.empty((self.E, 5), dtype=t.int32, device=self.device)
        _check(self.lib, self.lib.mcbs_sample_actions(self._h, int(bool(valid)), int(seed), int(step), out.data_ptr(), self._stream()),
               "mcbs_sample_actions")
        return out

    def decode_attacker_actions(self, multidiscrete=None, discrete=None, actions_out=None, invalid_out=None):
        """marlon's MultiDiscrete(10) / Discrete attacker actions -> engine rows [E,5] + invalid flags [E] (device)."""
        t = self.torch
        if (multidiscrete is None) == (discrete is None):
            raise ValueError("give exactly one of multidiscrete / discrete")
        src = multidiscrete if multidiscrete is not None else discrete
        src = src if isinstance(src, t.Tensor) else t.as_tensor(np.asarray(src))
        src = src.to(device=self.device, dtype=t.int64).contiguous()
        want = (self.E, 10) if multidiscrete is not None else (self.E,)
        if tuple(src.shape) != want:
            raise ValueError(f"expected shape {want}, got {tuple(src.shape)}")
        if actions_out is None:
            actions_out = t.empty((self.E, 5), dtype=t.int32, device=self.device)
        if invalid_out is None:
            invalid_out = t.empty(self.E, dtype=t.uint8, device=self.device)
        _check(self.lib, self.lib.mcbs_decode_attacker_actions(
            self._h, src.data_ptr() if multidiscrete is not None else None, src.data_ptr() if discrete is not None else None,
            actions_out.data_ptr(), invalid_out.data_ptr(), self._stream()), "mcbs_decode_attacker_actions")
        return actions_out, invalid_out

    def discrete_action_count(self) -> int:
        """Size of MaskedDiscreteAttackerWrapper's Discrete space: N*N*P*C + N*L + N*N*R (action_masking.py:74-80)."""
        return self._A

    def mask_logits(self, logits, fill: float = -1e8):
        """In place: logits[e, a] = mask(e, a) ? logits[e, a] : fill for the Discrete action mask of the LAST observation call
        (step_observe / observe / action_mask), rebuilt on the device from that call's per-env digest — the mask itself is never
        written.  logits: device float32 or bfloat16 [E, >= discrete_action_count()], rows contiguous."""
        _check(self.lib, self.lib.mcbs_mask_logits(self._h, *self._logits(logits, self.E, self._A), float(fill), self._stream()), "mcbs_mask_logits")
        return logits

    # -- bit-packed Discrete action masks (include/mcbs.h): int32 tensors [rows, row_words], bit a of a row = bit (a & 31) of word a >> 5 --
    def packed_mask_words(self):
        """-> (W, row_words): W = ceil(A / 32) words carry a row's mask; row_words = W rounded up to whole 16-byte groups (the rows
        pack_action_mask allocates)."""
        W = (self._A + 31) // 32
        return W, (W + 3) // 4 * 4

    def _packed_rows(self, bits, what: str, n=None):
        """bits: int32 rows of at least W words, the packed masks of n rows (None: any count)."""
        return self._rows(bits, (self.torch.int32,), what, n, (self._A + 31) // 32)

    def pack_action_mask(self, out=None):
        """The Discrete action mask of the LAST observation call as one bit per action, rebuilt on the device from that call's per-env
        digest (the preconditions of mask_logits).  out: device int32 [E, >= W] with contiguous rows (e.g. buffer[t] of a
        [T, E, row_words] rollout buffer), or None for a new zeroed [E, row_words] tensor.  Words from W on are not written."""
        t = self.torch
        if out is None:
            out = t.zeros((self.E, self.packed_mask_words()[1]), dtype=t.int32, device=self.device)
        self._packed_rows(out, "out", self.E)
        _check(self.lib, self.lib.mcbs_pack_action_mask(self._h, out.data_ptr(), _row_stride(out, self.E), self._stream()), "mcbs_pack_action_mask")
        return out

    def apply_packed_mask(self, bits, logits, fill: float = -1e8):
        """In place: logits[i, a] = bit(i, a) ? logits[i, a] : fill for every row i of bits [n, >= W] and logits float32 / bfloat16
        [n, >= A] (any n: a minibatch gathered from stored masks).  Write-only, like mask_logits; no digest involved."""
        n = self._packed_rows(bits, "bits").shape[0]
        lg = self._logits(logits, n, self._A)       # one row of logits per row of bits
        if n:
            _check(self.lib, self.lib.mcbs_apply_packed_mask(self._h, bits.data_ptr(), _row_stride(bits, n), *lg, n, float(fill), self._stream()),
                   "mcbs_apply_packed_mask")
        return logits

    def unpack_action_mask(self, bits, out=None):
        """bits [n, >= W] -> the bool mask [n, A] (out: device bool / uint8 [n, >= A] with contiguous rows; bytes from A on untouched)."""
        t = self.torch
        self._packed_rows(bits, "bits")
        n, A = bits.shape[0], self._A
        if out is None:
            out = t.empty((n, A), dtype=t.bool, device=self.device)
        self._rows(out, (t.bool, t.uint8), "out", n, A)            # one row per row of bits
        if n:
            _check(self.lib, self.lib.mcbs_unpack_action_mask(self._h, bits.data_ptr(), _row_stride(bits, n), out.data_ptr(), _row_stride(out, n),
                                                              n, self._stream()), "mcbs_unpack_action_mask")
        return out

    # -- action-mask keys (include/mcbs.h): int32 tensors [rows, >= Wk]; a key row expands to the packed mask of the step it was stored at --
    def mask_key_words(self) -> int:
        """Wk = 1 + ceil(Nk / 32) + ceil(Nk / 4): the words of one key row (mask_keys.key_words on the host)."""
        return self._Wk

    def _key_rows(self, keys, what: str, n=None):
        """keys: int32 rows of at least Wk words, the mask keys of n rows (None: any count)."""
        return self._rows(keys, (self.torch.int32,), what, n, self._Wk)

    def store_mask_keys(self, out=None):
        """The key of the Discrete action mask of the LAST observation call: the digest's counts and owned-source bits plus the
        discovery order, Wk words per env (the preconditions of pack_action_mask).  out: device int32 [E, >= Wk] with contiguous rows
        (e.g. buffer[t] of a [T, E, Wk] rollout buffer), or None for a new zeroed [E, Wk] tensor.  Words from Wk on are not written."""
        t = self.torch
        if out is None:
            out = t.zeros((self.E, self.mask_key_words()), dtype=t.int32, device=self.device)
        self._key_rows(out, "out", self.E)
        _check(self.lib, self.lib.mcbs_store_mask_keys(self._h, out.data_ptr(), _row_stride(out, self.E), self._stream()), "mcbs_store_mask_keys")
        return out

    def expand_mask_keys(self, keys, index=None, out=None):
        """Stored keys [n_source, >= Wk] -> the packed masks pack_action_mask would have written when they were stored, bit for bit:
        row i of the result is the mask of key row index[i] (index: device int64 [n]; an entry outside [0, n_source) gives a zero
        row) or, without an index, of key row i.  out: device int32 [n, >= W] with contiguous rows, or None for a new zeroed
        [n, row_words] tensor; words from W on are not written.  Reads no env state: works long after the envs have moved on, and
        under every defender kind."""
        t = self.torch
        self._key_rows(keys, "keys")
        idx, n = self._row_index(index, keys.shape[0])
        if out is None:
            out = t.zeros((n, self.packed_mask_words()[1]), dtype=t.int32, device=self.device)
        self._packed_rows(out, "out", n)
        if n:
            m = keys.shape[0]
            _check(self.lib, self.lib.mcbs_expand_mask_keys(self._h, keys.data_ptr(), _row_stride(keys, m), idx, m, out.data_ptr(),
                                                            _row_stride(out, n), n, self._stream()), "mcbs_expand_mask_keys")
        return out

    def _categorical_outputs(self, n, mode, actions, uniforms, out, bad_actions):
        """The checks and the out= handling the masked heads share: -> (actions, log_prob, entropy, n_allowed) to hand to the library."""
        t = self.torch
        if mode not in CATEGORICAL_MODES:
            raise ValueError(f"mode must be one of {sorted(CATEGORICAL_MODES)}, got {mode!r}")
        if out is not None and len(out) != 4:
            raise ValueError("out must be (actions, log_prob, entropy, n_allowed)")
        o_act, o_lp, o_ent, o_k = out if out is not None else (None, None, None, None)
        if mode == "evaluate":
            if actions is None:
                raise ValueError('mode="evaluate" needs actions (int64 [n])')
            o_act = self._arr(actions, t.int64, (n,), "actions")
        elif actions is not None:
            raise ValueError('actions are an input of mode="evaluate" only (preallocate outputs with out=)')
        else:
            o_act = self._arr(o_act, t.int64, (n,), "out.actions") if o_act is not None else t.empty(n, dtype=t.int64, device=self.device)
        o_lp = self._arr(o_lp, t.float32, (n,), "out.log_prob") if o_lp is not None else t.empty(n, dtype=t.float32, device=self.device)
        o_ent = self._arr(o_ent, t.float32, (n,), "out.entropy") if o_ent is not None else t.empty(n, dtype=t.float32, device=self.device)
        o_k = self._arr(o_k, t.int32, (n,), "out.n_allowed") if o_k is not None else t.empty(n, dtype=t.int32, device=self.device)
        if uniforms is not None:
            self._arr(uniforms, t.float32, (n,), "uniforms")
        if bad_actions is not None:
            self._counter(bad_actions, "bad_actions")
        return o_act, o_lp, o_ent, o_k

    # -- masked categorical head (include/mcbs.h): sample / log-prob / entropy of `Categorical(logits=where(mask, logits, -1e8))` --
    def masked_categorical(self, logits=None, *, bits=None, mode: str = "sample", actions=None, seed: int = 0, step: int = 0, uniforms=None,
                           out=None, bad_actions=None) -> MaskedCategorical:
        """MaskablePPO's action distribution in one launch, reading only the logits under set mask bits; logits are never modified.
        bits=None: the live form — one row per env, the mask of the LAST observation rebuilt from the digest (the preconditions of
        mask_logits), rows keyed by the global env id.  bits = packed masks int32 [n, >= W] (pack_action_mask's format): any n rows, no
        digest involved, rows keyed by their index.  logits: device float32 / bfloat16 [n, >= A] with contiguous rows, or None for the
        uniform law over the allowed actions.  mode: "sample" (inverse CDF in ascending action order), "argmax" (lowest index among equal
        logits) or "evaluate" (log-prob of the given `actions`, int64 [n]; NaN for an action outside [0, A), counted in bad_actions:
        optional device int32 [1], increased, not zeroed).  seed / step key the row's Philox number unless `uniforms` (device float32 [n]
        in [0, 1)) is given.  out: optional (actions, log_prob, entropy, n_allowed) of preallocated device tensors (int64, float32, float32,
        int32, each [n]).  -> MaskedCategorical(actions, log_prob, entropy, n_allowed)."""
        if mode not in CATEGORICAL_MODES:
            raise ValueError(f"mode must be one of {sorted(CATEGORICAL_MODES)}, got {mode!r}")
        if bits is not None:
            self._packed_rows(bits, "bits")
            n = bits.shape[0]
        else:
            n = self.E
        lg = self._logits(logits, n, self._A) if logits is not None else (None, 0, 0)          # None: the uniform law
        o_act, o_lp, o_ent, o_k = self._categorical_outputs(n, mode, actions, uniforms, out, bad_actions)
        common = (*lg, CATEGORICAL_MODES[mode], o_act.data_ptr(), o_lp.data_ptr(), o_ent.data_ptr(), o_k.data_ptr(), _ptr(uniforms), _u64(seed),
                  _u64(step), _ptr(bad_actions), self._stream())
        if bits is None:
            _check(self.lib, self.lib.mcbs_masked_categorical(self._h, *common), "mcbs_masked_categorical")
        elif n:
            _check(self.lib, self.lib.mcbs_masked_categorical_packed(self._h, bits.data_ptr(), _row_stride(bits, n), n, *common),
                   "mcbs_masked_categorical_packed")
        return MaskedCategorical(o_act, o_lp, o_ent, o_k)

    def masked_linear_categorical(self, latent, weight, bias=None, *, bits=None, mode: str = "sample", actions=None, seed: int = 0, step: int = 0,
                                  uniforms=None, out=None, bad_actions=None) -> MaskedCategorical:
        """masked_categorical without a logits tensor (mcbs_masked_linear_categorical): the logit of an ALLOWED action is computed in the
        kernel as bias[a] + latent[i] . weight[a], for a policy whose action_net is Linear(H, A).  latent: device float32 / bfloat16
        [n, H]; weight: [A, H] (torch.nn.Linear's layout), bias: [A] or None, all three of one dtype, last dimension contiguous,
        1 <= H <= 512.  bits, mode, actions, seed, step, uniforms, out, bad_actions and the result as for masked_categorical, whose outputs
        on logits holding the same values these are bit for bit; torch.nn.functional.linear sums in another order, so against it the
        logits agree to rounding.  This call builds no autograd graph: masked_linear_evaluate is mode="evaluate" with one."""
        if bits is not None:
            self._packed_rows(bits, "bits")
            n = bits.shape[0]
        else:
            n = self.E
        H = self._linear_head_inputs(latent, weight, bias, n)
        o_act, o_lp, o_ent, o_k = self._categorical_outputs(n, mode, actions, uniforms, out, bad_actions)
        common = (latent.data_ptr(), _row_stride(latent, n), weight.data_ptr(), _row_stride(weight, self._A), _ptr(bias), H, self._dtype_code(latent),
                  CATEGORICAL_MODES[mode], o_act.data_ptr(), o_lp.data_ptr(), o_ent.data_ptr(), o_k.data_ptr(), _ptr(uniforms), _u64(seed),
                  _u64(step), _ptr(bad_actions), self._stream())
        if bits is None:
            _check(self.lib, self.lib.mcbs_masked_linear_categorical(self._h, *common), "mcbs_masked_linear_categorical")
        elif n:
            _check(self.lib, self.lib.mcbs_masked_linear_categorical_packed(self._h, bits.data_ptr(), _row_stride(bits, n), n, *common),
                   "mcbs_masked_linear_categorical_packed")
        return MaskedCategorical(o_act, o_lp, o_ent, o_k)

    def _linear_head_inputs(self, latent, weight, bias, n) -> int:
        """The checks on (latent, weight, bias) the calls of the head from the latent share: -> H."""
        t = self.torch
        A = self._A
        for x, what in ((latent, "latent"), (weight, "weight")) + (((bias, "bias"),) if bias is not None else ()):
            if not isinstance(x, t.Tensor) or x.dtype not in (t.float32, t.bfloat16):
                raise ValueError(f"{what} must be a float32 or bfloat16 tensor")
            if x.device != self.device:
                raise ValueError(f"{what} must be on {self.device}, not {x.device}")
            if x.dtype != latent.dtype:
                raise ValueError(f"latent, weight and bias must have one dtype: latent is {latent.dtype}, {what} is {x.dtype}")
        if latent.dim() != 2 or latent.shape[0] != n or not 1 <= latent.shape[1] <= MCBS_LINEAR_MAX_H or latent.stride(1) != 1:
            raise ValueError(f"latent must be [{n}, H] with 1 <= H <= {MCBS_LINEAR_MAX_H} and contiguous rows")
        H = latent.shape[1]
        if weight.dim() != 2 or tuple(weight.shape) != (A, H) or weight.stride(1) != 1:
            raise ValueError(f"weight must be [{A}, {H}] (one row per Discrete action) with contiguous rows, got {tuple(weight.shape)}")
        if bias is not None and (tuple(bias.shape) != (A,) or not bias.is_contiguous()):
            raise ValueError(f"bias must be a contiguous [{A}] tensor")
        return H

    def masked_linear_categorical_grad_workspace(self, n: int, H: int) -> int:
        """The bytes of device workspace masked_linear_categorical_grad needs for n rows and a layer of width H."""
        return int(self.lib.mcbs_masked_linear_categorical_grad_workspace(self._h, int(n), int(H)))

    def masked_linear_categorical_grad(self, latent, weight, bias, bits, actions, grad_log_prob=None, grad_entropy=None, out=None,
                                       want=(True, True, True), workspace=None) -> MaskedLinearGrad:
        """The backward pass of masked_linear_categorical(bits=..., mode="evaluate") (mcbs_masked_linear_categorical_grad): the gradients of
        log_prob(actions) and the entropy with respect to latent [n, H], weight [A, H] and bias [A], given their incoming gradients
        grad_log_prob / grad_entropy (device float32 [n]; None = zeros), without an [n, A] tensor.  Inputs as in the forward (bias may be
        None: zeros; grad_bias is still the sum it would receive).  -> MaskedLinearGrad(grad_latent, grad_weight, grad_bias), float32
        whatever the inputs' dtype, every element written (dead rows and actions nobody allows: +0.0), bit-identical from call to call.
        want: which of the three to compute (None in the result for the others; without grad_weight and grad_bias the call is one launch
        instead of three).  out: optional (grad_latent, grad_weight, grad_bias) of preallocated device float32 tensors [n, >= H],
        [A, >= H] with contiguous rows and [A] contiguous, None entries are allocated; an entry given is computed whatever `want` says.
        workspace: an optional device uint8 tensor of at least masked_linear_categorical_grad_workspace(n, H) bytes; otherwise torch.empty."""
        t = self.torch
        if not isinstance(bits, t.Tensor):
            raise ValueError("bits must be a device int32 tensor [n, >= W] (the gradient exists in the packed form only)")
        self._packed_rows(bits, "bits")
        n = bits.shape[0]
        A = self._A
        H = self._linear_head_inputs(latent, weight, bias, n)
        self._grad_inputs(n, actions, (n,), grad_log_prob, grad_entropy)
        if out is not None and len(out) != 3:
            raise ValueError("out must be (grad_latent, grad_weight, grad_bias)")
        if len(want) != 3:
            raise ValueError("want must be three booleans: (grad_latent, grad_weight, grad_bias)")
        outs = []
        for k, (name, shape) in enumerate((("grad_latent", (n, H)), ("grad_weight", (A, H)), ("grad_bias", (A,)))):
            o = out[k] if out is not None else None
            if o is None:
                o = t.empty(shape, dtype=t.float32, device=self.device) if want[k] else None
            elif (not isinstance(o, t.Tensor) or o.dtype != t.float32 or o.device != self.device or o.dim() != len(shape) or o.shape[0] != shape[0]
                  or o.stride(-1) != 1 or (len(shape) == 2 and o.shape[1] < H)):
                raise ValueError(f"out.{name} must be a device float32 tensor {list(shape)} (rows may be longer) with contiguous rows")
            outs.append(o)
        if all(o is None for o in outs):
            raise ValueError("no gradient asked for: want is all False and out gives none")
        need = self.masked_linear_categorical_grad_workspace(n, H)
        if workspace is None:
            workspace = t.empty(need, dtype=t.uint8, device=self.device)
        elif (not isinstance(workspace, t.Tensor) or workspace.dtype != t.uint8 or workspace.device != self.device or not workspace.is_contiguous()
              or workspace.numel() < need):
            raise ValueError(f"workspace must be a contiguous device uint8 tensor of at least {need} bytes")
        g_lat, g_w, g_b = outs
        _check(self.lib, self.lib.mcbs_masked_linear_categorical_grad(
            self._h, bits.data_ptr(), _row_stride(bits, n), n, latent.data_ptr(), _row_stride(latent, n), weight.data_ptr(), _row_stride(weight, A),
            _ptr(bias), H, self._dtype_code(latent), actions.data_ptr(), _ptr(grad_log_prob), _ptr(grad_entropy), _ptr(g_lat), _row_stride(g_lat, n),
            _ptr(g_w), _row_stride(g_w, A), _ptr(g_b), workspace.data_ptr() if need else None, workspace.numel(), self._stream()),
            "mcbs_masked_linear_categorical_grad")
        return MaskedLinearGrad(g_lat, g_w, g_b)

    def masked_linear_evaluate(self, latent, weight, bias, bits, actions, bad_actions=None) -> MaskedCategorical:
        """masked_linear_categorical(bits=..., mode="evaluate") as a node of torch's autograd graph: the same numbers bit for bit, and
        log_prob and entropy carry a graph into latent, weight and bias, whose backward is one call of masked_linear_categorical_grad for
        the gradients autograd asks for (cast to the inputs' dtype); actions and n_allowed are not differentiable."""
        lp, ent, k = _masked_linear_evaluate_function(self.torch).apply(latent, weight, bias, self, bits, actions, bad_actions)
        return MaskedCategorical(actions, lp, ent, k)

    def masked_categorical_grad(self, logits, bits, actions, grad_log_prob=None, grad_entropy=None, out=None):
        """The backward pass of masked_categorical(bits=..., mode="evaluate") in one launch: the gradient with respect to `logits` of
        log_prob(actions) and the entropy, given their incoming gradients grad_log_prob / grad_entropy (device float32 [n]; None = zeros).
        logits float32 / bfloat16 [n, >= A], bits int32 [n, >= W], actions int64 [n] as in the forward.  out: a device tensor of the
        logits' dtype [n, >= A] with contiguous rows that does not overlap logits, or None for a new [n, A] one; columns [0, A) are
        written entirely (masked actions, all-zero rows and rows whose action lies outside [0, A): +0.0), columns from A on never.
        -> grad_logits."""
        t = self.torch
        if not isinstance(bits, t.Tensor):
            raise ValueError("bits must be a device int32 tensor [n, >= W] (the gradient exists in the packed form only)")
        self._packed_rows(bits, "bits")
        n = bits.shape[0]
        A = self._A
        lg = self._logits(logits, n, A)             # no None here: the uniform law has no gradient
        self._grad_inputs(n, actions, (n,), grad_log_prob, grad_entropy)
        out = self._grad_logits_out(out, logits, n, A)
        if n:
            _check(self.lib, self.lib.mcbs_masked_categorical_grad(
                self._h, bits.data_ptr(), _row_stride(bits, n), n, *lg, actions.data_ptr(), _ptr(grad_log_prob), _ptr(grad_entropy),
                out.data_ptr(), _row_stride(out, n), self._stream()), "mcbs_masked_categorical_grad")
        return out

    def _grad_inputs(self, n, actions, actions_shape, grad_log_prob, grad_entropy) -> None:
        """The checks the backward passes share: the forward's int64 actions and the two optional incoming gradients, float32 [n]."""
        t = self.torch
        self._arr(actions, t.int64, actions_shape, "actions")
        if grad_log_prob is not None:
            self._arr(grad_log_prob, t.float32, (n,), "grad_log_prob")
        if grad_entropy is not None:
            self._arr(grad_entropy, t.float32, (n,), "grad_entropy")

    def _grad_logits_out(self, out, logits, n, A):
        """out= of the two gradients with respect to logits: rows of the logits' dtype [n, >= A], or None for a new [n, A] tensor."""
        if out is None:
            return self.torch.empty((n, A), dtype=logits.dtype, device=self.device)
        return self._rows(out, (logits.dtype,), "out", n, A)

    def masked_evaluate(self, logits, bits, actions, bad_actions=None) -> MaskedCategorical:
        """masked_categorical(bits=..., mode="evaluate") as a node of torch's autograd graph: log_prob and entropy carry a graph into
        `logits`, whose backward is masked_categorical_grad (one launch each way); actions and n_allowed are not differentiable."""
        lp, ent, k = _masked_evaluate_function(self.torch).apply(logits, self, bits, actions, bad_actions)
        return MaskedCategorical(actions, lp, ent, k)

    # -- MultiDiscrete head (include/mcbs.h): sample / log-prob / entropy / gradient of SB3's MultiCategoricalDistribution --
    def _nvec_block(self, nvec):
        """nvec -> (host uint32 array for the library, D, A), cached per tuple; what the C side refuses (D outside [1, 16], an entry
        outside [1, 65 536]) is left to it."""
        key = tuple(int(v) for v in np.asarray(nvec).reshape(-1))
        hit = self._nvec_blocks.get(key)
        if hit is None:
            if any(v < 0 or v >= 2 ** 32 for v in key):
                raise ValueError(f"nvec entries must be unsigned 32-bit numbers, got {list(key)}")
            hit = self._nvec_blocks[key] = ((C.c_uint32 * max(len(key), 1))(*key), len(key), sum(key))
        return hit

    def multicategorical(self, logits, nvec, *, mode: str = "sample", actions=None, seed: int = 0, step: int = 0, uniforms=None,
                         row_key_base: int = 0, out=None, bad_actions=None) -> MultiCategorical:
        """PPO's action distribution over a MultiDiscrete(nvec) action in one launch: `split` by nvec, a Categorical per dimension,
        log_prob and entropy summed over the dimensions; logits are never modified.  logits: device float32 / bfloat16 [n, >= A] with
        contiguous rows, A = sum(nvec), any n; or None for the uniform law per dimension (n is then that of actions, uniforms or out,
        else n_envs).  nvec: up to 16 dimension widths, each in [1, 65 536].  mode: "sample" (per dimension inverse CDF in ascending index
        order), "argmax" (lowest index among equal logits) or "evaluate" (log-prob of the given `actions`, int64 [n, D]; NaN for a row with a
        component outside [0, nvec[d]), counted in bad_actions: optional device int32 [1], increased, not zeroed).  Row i is keyed by
        (seed, row_key_base + i, step), step < 2^48, unless `uniforms` (device float32 [n, D] in [0, 1)) is given.  out: optional
        (actions, log_prob, entropy) of preallocated contiguous device tensors (int64 [n, D], float32 [n], float32 [n]).
        -> MultiCategorical(actions, log_prob, entropy)."""
        t = self.torch
        if mode not in CATEGORICAL_MODES:
            raise ValueError(f"mode must be one of {sorted(CATEGORICAL_MODES)}, got {mode!r}")
        block, D, A = self._nvec_block(nvec)
        if out is not None and len(out) != 3:
            raise ValueError("out must be (actions, log_prob, entropy)")
        o_act, o_lp, o_ent = out if out is not None else (None, None, None)
        # This method's wall time at 64 rows is mostly Python, and each helper call is 50 ns of it: what _logits, _action_rows, _ptr and
        # _u64 do elsewhere is written out here.  The checks themselves (_rows, _arr, _counter) and the stride rule (_row_stride) are shared.
        if logits is not None:
            n = self._rows(logits, (t.float32, t.bfloat16), "logits", None, A).shape[0]
            lg = (logits.data_ptr(), 0 if logits.dtype == t.float32 else 1, _row_stride(logits, n))
        else:                                       # the uniform law
            given = [x for x in (actions, uniforms, o_act, o_lp, o_ent) if isinstance(x, t.Tensor) and x.dim() >= 1]
            lg, n = (None, 0, 0), given[0].shape[0] if given else self.E
        if mode == "evaluate":
            if actions is None:
                raise ValueError('mode="evaluate" needs actions (int64 [n, D])')
            o_act = self._arr(actions, t.int64, (n, D), "actions")
        elif actions is not None:
            raise ValueError('actions are an input of mode="evaluate" only (preallocate outputs with out=)')
        else:
            o_act = self._arr(o_act, t.int64, (n, D), "out.actions") if o_act is not None else t.empty((n, D), dtype=t.int64, device=self.device)
        o_lp = self._arr(o_lp, t.float32, (n,), "out.log_prob") if o_lp is not None else t.empty(n, dtype=t.float32, device=self.device)
        o_ent = self._arr(o_ent, t.float32, (n,), "out.entropy") if o_ent is not None else t.empty(n, dtype=t.float32, device=self.device)
        if uniforms is not None:
            self._arr(uniforms, t.float32, (n, D), "uniforms")
        if bad_actions is not None:
            self._counter(bad_actions, "bad_actions")
        _check(self.lib, self.lib.mcbs_multicategorical(
            self._h, block, D, n, *lg, CATEGORICAL_MODES[mode], o_act.data_ptr(), o_lp.data_ptr(), o_ent.data_ptr(),
            uniforms.data_ptr() if uniforms is not None else None, int(seed) & _U64, int(step) & _U64, int(row_key_base) & _U64,
            bad_actions.data_ptr() if bad_actions is not None else None, self._stream()), "mcbs_multicategorical")
        return MultiCategorical(o_act, o_lp, o_ent)

    def multicategorical_grad(self, logits, nvec, actions, grad_log_prob=None, grad_entropy=None, out=None):
        """The backward pass of multicategorical(mode="evaluate") in one launch: the gradient with respect to `logits` of log_prob(actions)
        and the entropy, given their incoming gradients grad_log_prob / grad_entropy (device float32 [n]; None = zeros).  logits float32 /
        bfloat16 [n, >= A], actions int64 [n, D] as in the forward.  out: a device tensor of the logits' dtype [n, >= A] with contiguous
        rows that does not overlap logits, or None for a new [n, A] one; columns [0, A) are written entirely (a row with a component
        outside its range: +0.0), columns from A on never.  -> grad_logits."""
        block, D, A = self._nvec_block(nvec)
        lg = self._logits(logits, None, A)          # no None here: the uniform law has no gradient
        n = logits.shape[0]
        self._grad_inputs(n, actions, (n, D), grad_log_prob, grad_entropy)
        out = self._grad_logits_out(out, logits, n, A)
        _check(self.lib, self.lib.mcbs_multicategorical_grad(
            self._h, block, D, n, *lg, actions.data_ptr(), _ptr(grad_log_prob), _ptr(grad_entropy), out.data_ptr(), _row_stride(out, n),
            self._stream()), "mcbs_multicategorical_grad")
        return out

    def multicategorical_evaluate(self, logits, nvec, actions, bad_actions=None) -> MultiCategorical:
        """multicategorical(mode="evaluate") as a node of torch's autograd graph: log_prob and entropy carry a graph into `logits`, whose
        backward is multicategorical_grad (one launch each way); actions are not differentiable."""
        lp, ent = _multicategorical_evaluate_function(self.torch).apply(logits, self, tuple(int(v) for v in np.asarray(nvec).reshape(-1)),
                                                                        actions, bad_actions)
        return MultiCategorical(actions, lp, ent)

    # -- generalized advantage estimation (include/mcbs.h): advantages and returns of a whole [T, E] rollout in one launch --
    def gae(self, rewards, values, episode_starts, last_values, last_dones, gamma: float, gae_lambda: float, bootstrap=None, advantages=None,
            returns=None):
        """Stable-Baselines3's RolloutBuffer.compute_returns_and_advantage on the device, one launch, bit for bit its float32 loop (the
        operation order is in include/mcbs.h).  rewards, values float32 [T, E] and episode_starts uint8 [T, E] (nonzero = start) are device
        tensors with unit inner stride: dense, or [T, :E] views of wider buffers, each with its own row stride; last_values float32 [E],
        last_dones uint8 [E], contiguous.  bootstrap: optional float32 [T, E], the terminal observation's value where step t was truncated and
        0 elsewhere (rewards + gamma * bootstrap replaces rewards; without it those two operations are not done at all).  advantages /
        returns: preallocated float32 [T, E] outputs of the same kind, allocated when None; they may not overlap an input or each other
        (McbsError).  E is the call's own: any producer's buffer is served.  -> (advantages, returns)."""
        t = self.torch

        def rows(x, dtype, what, shape=None):
            if not isinstance(x, t.Tensor) or x.dtype != dtype or x.device != self.device:
                raise ValueError(f"{what} must be a device {dtype} tensor on {self.device}")
            if x.dim() != 2 or (shape is not None and tuple(x.shape) != shape):
                raise ValueError(f"{what} must have shape [T, E]" + (f" = {list(shape)}" if shape is not None else "") + f", got {list(x.shape)}")
            # the C side sees only the row stride: the elements of a row must be adjacent, and rows of a [T, :E] view at least E apart
            if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.shape[1] > 0 and x.stride(0) < x.shape[1]:
                raise ValueError(f"{what} must have unit inner stride and rows at least E elements apart (strides {x.stride()})")
            return x

        rows(rewards, t.float32, "rewards")
        T, E = rewards.shape
        shape = (T, E)
        rows(values, t.float32, "values", shape)
        rows(episode_starts, t.uint8, "episode_starts", shape)
        self._arr(last_values, t.float32, (E,), "last_values")
        self._arr(last_dones, t.uint8, (E,), "last_dones")
        if bootstrap is not None:
            rows(bootstrap, t.float32, "bootstrap", shape)
        advantages = t.empty(shape, dtype=t.float32, device=self.device) if advantages is None else rows(advantages, t.float32, "advantages", shape)
        returns = t.empty(shape, dtype=t.float32, device=self.device) if returns is None else rows(returns, t.float32, "returns", shape)
        io = GaeIO(rewards.data_ptr(), values.data_ptr(), episode_starts.data_ptr(), _ptr(bootstrap), last_values.data_ptr(), last_dones.data_ptr(),
                   advantages.data_ptr(), returns.data_ptr(), T, E, _row_stride(rewards, T), _row_stride(values, T), _row_stride(episode_starts, T),
                   _row_stride(bootstrap, T), _row_stride(advantages, T), _row_stride(returns, T), float(gamma), float(gae_lambda))
        _check(self.lib, self.lib.mcbs_gae(self._h, C.byref(io), self._stream()), "mcbs_gae")
        return advantages, returns

    # -- feature encoder (include/mcbs.h): observation rows -> the one-hot float rows a policy's first layer takes --
    def feature_layout(self, layout) -> FeatureLayoutHandle:
        """Hand a `features.FeatureLayout` (built for this engine's topology and bounds) to the library; the handle is what
        encode_features takes.  Descriptors are checked and uploaded once."""
        d = np.ascontiguousarray(layout.descriptors, dtype=np.uint32)
        r = np.ascontiguousarray(layout.mask_ranges, dtype=np.uint32).reshape(-1, 3)
        h = C.c_void_p()
        rc = self.lib.mcbs_feature_layout_create(self._h, d.ctypes.data if d.size else None, d.size, r.ctypes.data if r.size else None,
                                                 r.shape[0], C.byref(h))
        _check(self.lib, rc, "mcbs_feature_layout_create")
        handle = FeatureLayoutHandle(self.lib, h, layout)
        if handle.width != layout.width:
            raise McbsError(f"feature layout: the library counts {handle.width} columns, the layout {layout.width}")
        return handle

    def _feature_out(self, handle: FeatureLayoutHandle, n: int, out, dtype, out_of_range):
        """The out= / dtype= / out_of_range= handling the two feature encoders share -> (out [n, >= F], MCBS_FEATURES_* code)."""
        t = self.torch
        F = handle.width
        if out is None:
            dtype = dtype or t.float32
            if dtype not in self._feature_dtypes:
                raise ValueError("features dtype must be float32, bfloat16 or float16")
            out = t.empty((n, handle.layout.padded_width(self._feature_dtypes[dtype][1])), dtype=dtype, device=self.device)
        if out.dtype not in self._feature_dtypes:
            raise ValueError("out must be float32, bfloat16 or float16")
        code = self._feature_dtypes[out.dtype][0]
        if dtype is not None and out.dtype != dtype:
            raise ValueError(f"out is {out.dtype}, dtype asks for {dtype}")
        self._rows(out, (out.dtype,), "out", n, F)
        if out_of_range is not None:
            self._counter(out_of_range, "out_of_range")
        return out, code

    def _int_fields(self, obs: dict, all_five: bool):
        """The observation's int32 fields in `obs` as contiguous device tensors with a leading row axis -> (ObsBuffers block, rows n)."""
        t = self.torch
        ptrs, n = {}, None
        for k, per_row in self._feature_rows.items():
            v = obs.get(k)
            if v is None:
                if all_five:
                    raise ValueError(f"obs lacks {k!r}: all five int32 fields are packed")
                continue
            if v.dtype != t.int32 or v.device != self.device or not v.is_contiguous() or v.dim() < 1 or v.numel() != v.shape[0] * per_row:
                raise ValueError(f"obs[{k!r}] must be a contiguous device int32 tensor of {per_row} values per row")
            if n is None:
                n = v.shape[0]
            elif v.shape[0] != n:
                raise ValueError(f"obs[{k!r}] has {v.shape[0]} rows, other fields {n}")
            ptrs[k] = v.data_ptr()
        if n is None:
            raise ValueError("obs holds none of the observation's int32 fields")
        return ObsBuffers(**ptrs), n

    def encode_features(self, handle: FeatureLayoutHandle, obs: dict, bits=None, out=None, dtype=None, out_of_range=None):
        """Feature rows [n, F] of n observation rows, one launch (mcbs_encode_features).  obs: the int32 fields `scalars`,
        `leaked_credentials`, `credential_cache_matrix`, `discovered_nodes_properties`, `nodes_privilegelevel` as contiguous device
        tensors with a leading row axis n — the live observation (n = E) or rows gathered from a rollout buffer (any n); a field the
        layout does not read may be missing.  bits: packed masks int32 [n, >= W] (pack_action_mask's format), needed when the layout has
        mask columns.  out: device float32 / bfloat16 / float16 [n, >= F] with contiguous rows (columns from F on are not touched), or
        None for a new tensor of `dtype` (default float32) whose rows are padded to whole 128-byte lines; returns the [n, F] view.
        Every column below F is written.  out_of_range: optional device int32 [1]; the number of elements whose value lay outside its
        class count is ADDED to it (such an element's columns are all zero)."""
        fields, n = self._int_fields(obs, all_five=False)
        if handle.has_masks:
            if bits is None:
                raise ValueError("the layout has mask columns: bits (packed action masks [n, >= W]) is required")
            self._packed_rows(bits, "bits", n)
        else:
            bits = None                             # read by a layout with mask columns only
        out, code = self._feature_out(handle, n, out, dtype, out_of_range)
        if n:
            _check(self.lib, self.lib.mcbs_encode_features(self._h, handle.ptr, C.byref(fields), _ptr(bits), _row_stride(bits, n), out.data_ptr(), code,
                                                           _row_stride(out, n), n, _ptr(out_of_range), self._stream()), "mcbs_encode_features")
        return out[:, :handle.width]

    # -- packed observations (include/mcbs.h): int32 tensors [rows, >= W_obs], every value of the five fields a bit field --
    def observation_packing(self, packing) -> ObservationPackingHandle:
        """Hand a `features.ObservationPacking` (built for this engine's topology and bounds) to the library; the handle is what
        pack_observation / unpack_observation / encode_features_packed take.  The library derives word and shift itself."""
        v = np.ascontiguousarray(packing.valid_codes, dtype=np.uint32)
        h = C.c_void_p()
        _check(self.lib, self.lib.mcbs_obs_packing_create(self._h, v.ctypes.data, v.size, C.byref(h)), "mcbs_obs_packing_create")
        handle = ObservationPackingHandle(self.lib, h, packing)
        if handle.words != packing.words:
            raise McbsError(f"observation packing: the library counts {handle.words} words per row, the host mirror {packing.words}")
        return handle

    def _packed_obs_rows(self, x, handle: ObservationPackingHandle, what: str, n=None):
        """x: int32 rows of at least W_obs words, n packed observations (None: any count)."""
        return self._rows(x, (self.torch.int32,), what, n, handle.words)

    def _row_index(self, index, n_source: int, what: str = "index"):
        """-> (pointer or None, rows asked): index int64 [n] on the device, or None for rows 0 .. n_source - 1"""
        t = self.torch
        if index is None:
            return None, n_source
        if index.dtype != t.int64 or index.dim() != 1 or index.device != self.device or not index.is_contiguous():
            raise ValueError(f"{what} must be a contiguous device int64 tensor [n]")
        return index.data_ptr(), index.shape[0]

    def pack_observation(self, handle: ObservationPackingHandle, obs: dict, out=None, out_of_range=None):
        """The five int32 fields of n observation rows (as encode_features takes them, all five required) as packed rows, one launch
        (mcbs_pack_observation).  out: device int32 [n, >= W_obs] with contiguous rows, e.g. `buf.observations["packed"][buf.pos]` of a
        rollout buffer (words from W_obs on are not touched, every word below is written), or None for a new [n, W_obs] tensor.
        out_of_range: optional device int32 [1]; the number of values stored as their out-of-range code is ADDED to it."""
        t = self.torch
        fields, n = self._int_fields(obs, all_five=True)
        if out is None:
            out = t.empty((n, handle.words), dtype=t.int32, device=self.device)
        self._packed_obs_rows(out, handle, "out", n)
        if out_of_range is not None:
            self._counter(out_of_range, "out_of_range")
        if n:
            _check(self.lib, self.lib.mcbs_pack_observation(self._h, handle.ptr, C.byref(fields), out.data_ptr(), _row_stride(out, n), n,
                                                            _ptr(out_of_range), self._stream()), "mcbs_pack_observation")
        return out

    def unpack_observation(self, handle: ObservationPackingHandle, packed, index=None, out=None):
        """Packed rows [m, >= W_obs] -> dict of the five int32 fields in their own shapes (mcbs_unpack_observation).  index: optional
        device int64 [n]: output row i is stored row index[i] (an index outside [0, m) reads nothing: that row's values are their
        out-of-range codes); without it n = m.  out: dict of contiguous device int32 tensors with n rows for the fields wanted (None:
        all five, newly allocated)."""
        t = self.torch
        self._packed_obs_rows(packed, handle, "packed")
        idx, n = self._row_index(index, packed.shape[0])
        if out is None:
            out = {k: t.empty((n,) + self._shapes[k][0], dtype=t.int32, device=self.device) for k in FEATURE_FIELDS}
        ptrs = {}
        for k, v in out.items():
            per_row = self._feature_rows.get(k)
            if per_row is None:
                raise ValueError(f"out[{k!r}] is not one of the observation's int32 fields")
            if v.dtype != t.int32 or v.device != self.device or not v.is_contiguous() or v.dim() < 1 or v.shape[0] != n or v.numel() != n * per_row:
                raise ValueError(f"out[{k!r}] must be a contiguous device int32 tensor of {n} rows of {per_row} values")
            ptrs[k] = v.data_ptr()
        if n and ptrs:
            _check(self.lib, self.lib.mcbs_unpack_observation(self._h, handle.ptr, packed.data_ptr(), _row_stride(packed, packed.shape[0]), idx, packed.shape[0], n,
                                                              C.byref(ObsBuffers(**ptrs)), self._stream()), "mcbs_unpack_observation")
        return out

    def encode_features_packed(self, feature_handle: FeatureLayoutHandle, packing_handle: ObservationPackingHandle, packed, bits=None, index=None,
                               out=None, dtype=None, out_of_range=None):
        """encode_features from packed rows [m, >= W_obs] (mcbs_encode_features_packed), one launch, the same outputs and the same out=
        / dtype= / out_of_range= rules.  bits: packed masks int32 [m, >= W], row for row with `packed`, needed when the layout has mask
        columns.  index: optional device int64 [n]: output row i is built from row index[i] of BOTH packed and bits — pass a rollout
        buffer's whole [T * E, ...] storage and a minibatch's row index, nothing is gathered first.  An index outside [0, m) reads
        nothing: that row is all zero and out_of_range grows by the layout's element count."""
        self._packed_obs_rows(packed, packing_handle, "packed")
        m = packed.shape[0]
        idx, n = self._row_index(index, m)
        if feature_handle.has_masks:
            if bits is None:
                raise ValueError("the layout has mask columns: bits (packed action masks [m, >= W]) is required")
            self._packed_rows(bits, "bits", m)
        else:
            bits = None                             # read by a layout with mask columns only
        out, code = self._feature_out(feature_handle, n, out, dtype, out_of_range)
        if n:
            _check(self.lib, self.lib.mcbs_encode_features_packed(
                self._h, feature_handle.ptr, packing_handle.ptr, packed.data_ptr(), _row_stride(packed, m), _ptr(bits), _row_stride(bits, m), idx, m,
                out.data_ptr(), code, _row_stride(out, n), n, _ptr(out_of_range), self._stream()), "mcbs_encode_features_packed")
        return out[:, :feature_handle.width]

    # -- the first layer from the observation (include/mcbs.h): Linear(F, H) on the feature row without the feature row --
    def _first_layer_source(self, handle: FeatureLayoutHandle, obs, packing, packed, index):
        """The source of the three first-layer calls: EITHER obs (the dense int32 fields, as encode_features takes them) OR packing +
        packed (+ index), as encode_features_packed takes them -> (obs block or None, packing pointer, packed pointer, packed row
        stride, index pointer, source rows, rows n, the tensors kept alive)."""
        if handle.has_masks:
            raise ValueError("the layout has mask columns: the first-layer calls serve layouts without them (include_masks is out of scope)")
        if (obs is None) == (packed is None):
            raise ValueError("give either obs= (the dense int32 fields) or packing= and packed= (stored packed rows)")
        if obs is not None:
            if packing is not None or index is not None:
                raise ValueError("packing= and index= belong to packed=: the dense fields are read row for row")
            fields, n = self._int_fields(obs, all_five=False)
            return fields, None, None, 0, None, 0, n
        if not isinstance(packing, ObservationPackingHandle):
            raise ValueError("packed= needs packing=, the handle of observation_packing()")
        self._packed_obs_rows(packed, packing, "packed")
        m = packed.shape[0]
        idx, n = self._row_index(index, m)
        return None, packing.ptr, packed.data_ptr(), _row_stride(packed, m), idx, m, n

    def _first_layer_weight(self, handle: FeatureLayoutHandle, weight_t, bias) -> int:
        """weight_t [F, H] (rows may lie further apart) and bias [H] or None, float32 or bfloat16, one dtype -> H"""
        t = self.torch
        self._rows(weight_t, (t.float32, t.bfloat16), "weight_t", handle.width, 1)
        H = weight_t.shape[1]
        if H > MCBS_LINEAR_MAX_H:
            raise ValueError(f"weight_t is [F, H = {H}]: H is at most {MCBS_LINEAR_MAX_H}")
        if bias is not None:
            self._arr(bias, weight_t.dtype, (H,), "bias")
        return H

    def first_layer(self, handle: FeatureLayoutHandle, weight_t, bias=None, *, obs=None, packing=None, packed=None, index=None, out=None,
                    dtype=None, out_of_range=None):
        """torch.nn.functional.linear(encode_features(...), weight_t.T, bias) without the feature rows, one launch (mcbs_first_layer /
        mcbs_first_layer_packed): out[i] = bias + the weight column every one-hot element of row i selects, one float32 accumulator, the
        elements in row order.  handle: a feature_layout() without mask columns.  weight_t: device float32 / bfloat16 [F, H] with
        contiguous rows (rows may lie further apart) — the TRANSPOSE of torch's Linear.weight; bias [H] of the same dtype or None.
        Source: obs= the int32 fields with a leading row axis (as encode_features), or packing= + packed= [m, >= W_obs] (+ index= device
        int64 [n]: output row i is stored row index[i]; an index outside [0, m) gives the bias alone).  out: device float32 / bfloat16
        [n, >= H] with contiguous rows (columns from H on are not touched), or None for a new [n, H] tensor of `dtype` (default float32;
        independent of the weights' dtype); returns the [n, H] view.  out_of_range: optional device int32 [1]; the number of elements
        whose value lay outside its class count (they select nothing) is ADDED to it."""
        t = self.torch
        fields, pk, pp, prs, idx, m, n = self._first_layer_source(handle, obs, packing, packed, index)
        H = self._first_layer_weight(handle, weight_t, bias)
        if out is None:
            out = t.empty((n, H), dtype=dtype or t.float32, device=self.device)
        if out.dtype not in (t.float32, t.bfloat16) or (dtype is not None and out.dtype != dtype):
            raise ValueError(f"out must be float32 or bfloat16{'' if dtype is None else f' and of dtype {dtype}'}, got {_describe(out)}")
        self._rows(out, (out.dtype,), "out", n, H)
        if out_of_range is not None:
            self._counter(out_of_range, "out_of_range")
        tail = (weight_t.data_ptr(), _row_stride(weight_t, handle.width), _ptr(bias), self._dtype_code(weight_t), H, out.data_ptr(),
                self._dtype_code(out), _row_stride(out, n), _ptr(out_of_range), self._stream())
        if fields is not None:
            _check(self.lib, self.lib.mcbs_first_layer(self._h, handle.ptr, C.byref(fields), n, *tail), "mcbs_first_layer")
        else:
            _check(self.lib, self.lib.mcbs_first_layer_packed(self._h, handle.ptr, pk, pp, prs, idx, m, n, *tail), "mcbs_first_layer_packed")
        return out[:, :H]

    def first_layer_grad_workspace(self, handle: FeatureLayoutHandle, n: int, H: int) -> int:
        """The bytes of device workspace first_layer_grad needs for n rows and a layer of width H."""
        return int(self.lib.mcbs_first_layer_grad_workspace(self._h, handle.ptr, int(n), int(H)))

    def first_layer_grad(self, handle: FeatureLayoutHandle, grad_out, *, obs=None, packing=None, packed=None, index=None, out=None,
                         want=(True, True), workspace=None) -> FirstLayerGrad:
        """The backward pass of first_layer (mcbs_first_layer_grad), two launches: grad_weight_t [F, H] — every row's grad_out added into
        the weight columns that row selected — and grad_bias [H], from grad_out, a device float32 [n, >= H'] tensor with contiguous rows
        whose width is H, and the same source the forward took (obs=, or packing= + packed= + index=).  -> FirstLayerGrad(grad_weight_t,
        grad_bias), float32, every element written (a column no row selects: +0.0), bit-identical from call to call.  want: which of the
        two to compute (None in the result for the other).  out: optional (grad_weight_t, grad_bias) of preallocated device float32
        tensors [F, >= H] with contiguous rows and [H] contiguous; None entries are allocated, an entry given is computed whatever `want`
        says.  workspace: an optional device uint8 tensor of at least first_layer_grad_workspace(handle, n, H) bytes; otherwise
        torch.empty."""
        t = self.torch
        fields, pk, pp, prs, idx, m, n = self._first_layer_source(handle, obs, packing, packed, index)
        self._rows(grad_out, (t.float32,), "grad_out", n, 1)
        H, F = grad_out.shape[1], handle.width
        if H > MCBS_LINEAR_MAX_H:
            raise ValueError(f"grad_out is [n, H = {H}]: H is at most {MCBS_LINEAR_MAX_H}")
        if (out is not None and len(out) != 2) or len(want) != 2:
            raise ValueError("out must be (grad_weight_t, grad_bias) and want two booleans")
        g_w, g_b = out if out is not None else (None, None)
        if g_w is None:
            g_w = t.empty((F, H), dtype=t.float32, device=self.device) if want[0] else None
        else:
            self._rows(g_w, (t.float32,), "out.grad_weight_t", F, H)
        if g_b is None:
            g_b = t.empty((H,), dtype=t.float32, device=self.device) if want[1] else None
        else:
            self._arr(g_b, t.float32, (H,), "out.grad_bias")
        if g_w is None and g_b is None:
            raise ValueError("no gradient asked for: want is all False and out gives none")
        need = self.first_layer_grad_workspace(handle, n, H)
        if workspace is None:
            workspace = t.empty(need, dtype=t.uint8, device=self.device)
        elif (not isinstance(workspace, t.Tensor) or workspace.dtype != t.uint8 or workspace.device != self.device or not workspace.is_contiguous()
              or workspace.numel() < need):
            raise ValueError(f"workspace must be a contiguous device uint8 tensor of at least {need} bytes")
        _check(self.lib, self.lib.mcbs_first_layer_grad(
            self._h, handle.ptr, None if fields is None else C.byref(fields), pk, pp, prs, idx, m, n, grad_out.data_ptr(), _row_stride(grad_out, n), H,
            _ptr(g_w), _row_stride(g_w, F), _ptr(g_b), workspace.data_ptr() if need else None, workspace.numel(), self._stream()),
            "mcbs_first_layer_grad")
        return FirstLayerGrad(None if g_w is None else g_w[:, :H], g_b)

    def first_layer_evaluate(self, handle: FeatureLayoutHandle, weight, bias=None, *, obs=None, packing=None, packed=None, index=None, dtype=None,
                             out_of_range=None, weight_t=None):
        """first_layer as a node of torch's autograd graph, taking torch's own parameters: weight [H, F] (Linear.weight) and bias [H].
        Forward transposes once (weight.t().contiguous(); or pass weight_t=, a transposed copy made once per update) and calls
        first_layer: the same bits.  Backward casts the upstream gradient to contiguous float32, calls first_layer_grad once for the
        gradients autograd asks for and returns them in the parameters' shapes ([H, F], [H]) and dtypes; the integer inputs have no
        gradient."""
        t = self.torch
        if not isinstance(weight, t.Tensor) or weight.dim() != 2 or weight.shape[1] != handle.width:
            raise ValueError(f"weight must be torch's Linear.weight [H, F = {handle.width}], got {_describe(weight)}")
        source = dict(obs=obs, packing=packing, packed=packed, index=index)
        return _first_layer_evaluate_function(t).apply(weight, bias, self, handle, source, dtype, out_of_range, weight_t)

    # -- learned defender (batches created with defender=("external",)) --
    def alloc_defender_obs(self) -> dict:
        t, N, S = self.torch, self.topo.n_nodes, int(self.topo.header()["n_services"])
        mk = lambda n: t.zeros((self.E, n), dtype=t.int8, device=self.device)
        return dict(infected_nodes=mk(N), incoming_firewall_status=mk(6 * N), outgoing_firewall_status=mk(6 * N), services_status=mk(S))

    def defender_step(self, actions12, obs: Optional[dict] = None, out=None):
        """DefenderEnvWrapper's validity check + LearningDefender.executeAction for every env.
        -> (valid u8 [E], availability f64 [E], evicted u8 [E]) device tensors (`out`: that triple, caller-owned; default: the engine's own
        buffers, overwritten by the next call)."""
        t = self.torch
        a = actions12 if isinstance(actions12, t.Tensor) else t.as_tensor(np.asarray(actions12))
        a = a.to(device=self.device, dtype=t.int64).contiguous()
        if tuple(a.shape) != (self.E, 12):
            raise ValueError(f"defender actions must have shape ({self.E}, 12), got {tuple(a.shape)}")
        if not hasattr(self, "_def_out"):
            self._def_out = (t.zeros(self.E, dtype=t.uint8, device=self.device), t.zeros(self.E, dtype=t.float64, device=self.device),
                             t.zeros(self.E, dtype=t.uint8, device=self.device))
        v, av, ev = self._def_out if out is None else out
        o = DefenderObs(**{k: x.data_ptr() for k, x in obs.items()}) if obs is not None else None
        _check(self.lib, self.lib.mcbs_defender_step(self._h, a.data_ptr(), v.data_ptr(), av.data_ptr(), ev.data_ptr(),
                                                     C.byref(o) if o is not None else None, self._stream()), "mcbs_defender_step")
        return v, av, ev

    def defender_observe(self, obs: dict) -> dict:
        o = DefenderObs(**{k: x.data_ptr() for k, x in obs.items()})
        _check(self.lib, self.lib.mcbs_defender_observe(self._h, C.byref(o), self._stream()), "mcbs_defender_observe")
        return obs

    # -- packed defender observations (include/mcbs.h): int32 tensors [rows, >= W_def], one bit per MultiBinary element --
    def defender_obs_words(self) -> int:
        """W_def, the uint32 words of a packed defender row (mcbs_defender_obs_words); 0 for a batch without a learned defender."""
        return int(self.lib.mcbs_defender_obs_words(self._h))

    def _defender_field_sizes(self) -> dict:
        N, S = self.topo.n_nodes, int(self.topo.header()["n_services"])
        return dict(infected_nodes=N, incoming_firewall_status=6 * N, outgoing_firewall_status=6 * N, services_status=S)

    def _defender_packed_rows(self, x, what: str, n=None):
        """x: int32 rows of at least W_def words, n packed defender observations (None: any count)."""
        return self._rows(x, (self.torch.int32,), what, n, self.defender_obs_words())

    def _defender_dense(self, obs: dict, what: str, n=None, partial: bool = False):
        """The four int8 fields of `obs` as contiguous device tensors of n rows (None: taken from the first) -> (DefenderObs block, n);
        partial: fields may be missing (skipped), but none unknown."""
        t = self.torch
        sizes = self._defender_field_sizes()
        unknown = [k for k in obs if k not in sizes]
        if unknown or (not partial and len(obs) != len(sizes)):
            raise ValueError(f"{what} holds the four int8 fields {sorted(sizes)}" + (f", not {unknown}" if unknown else ""))
        ptrs = {}
        for k, x in obs.items():
            if n is None:
                n = x.shape[0] if isinstance(x, t.Tensor) and x.dim() >= 1 else None
            self._arr(x, t.int8, (n, sizes[k]), f"{what}[{k!r}]")
            ptrs[k] = x.data_ptr()
        return DefenderObs(**ptrs), n

    def defender_observe_packed(self, out=None):
        """The packed rows of the live state of all envs, one launch (mcbs_defender_observe_packed).  out: device int32 [E, >= W_def]
        with contiguous rows (words from W_def on are not touched, every word below is written), or None for a new [E, W_def] tensor."""
        if out is None:
            out = self.torch.empty((self.E, self.defender_obs_words()), dtype=self.torch.int32, device=self.device)
        self._defender_packed_rows(out, "out", self.E)
        _check(self.lib, self.lib.mcbs_defender_observe_packed(self._h, out.data_ptr(), _row_stride(out, self.E), self._stream()),
               "mcbs_defender_observe_packed")
        return out

    def pack_defender_observation(self, obs: dict, out=None):
        """n dense rows of the four int8 fields (a dict as alloc_defender_obs builds it, any n) as packed rows, one launch
        (mcbs_pack_defender_observation): a bit is set where the element is not zero.  out: device int32 [n, >= W_def] or None."""
        block, n = self._defender_dense(obs, "obs")
        if out is None:
            out = self.torch.empty((n, self.defender_obs_words()), dtype=self.torch.int32, device=self.device)
        self._defender_packed_rows(out, "out", n)
        if n:
            _check(self.lib, self.lib.mcbs_pack_defender_observation(self._h, C.byref(block), n, out.data_ptr(), _row_stride(out, n), self._stream()),
                   "mcbs_pack_defender_observation")
        return out

    def unpack_defender_observation(self, packed, index=None, out=None):
        """Packed rows [m, >= W_def] -> dict of the four int8 fields, 0 / 1 (mcbs_unpack_defender_observation).  index: optional device
        int64 [n]: output row i is stored row index[i] (an index outside [0, m) reads nothing: that row is all zero); without it n = m.
        out: dict of contiguous device int8 tensors of n rows for the fields wanted (None: all four, newly allocated)."""
        t = self.torch
        self._defender_packed_rows(packed, "packed")
        m = packed.shape[0]
        idx, n = self._row_index(index, m)
        if out is None:
            out = {k: t.empty((n, s), dtype=t.int8, device=self.device) for k, s in self._defender_field_sizes().items()}
        block, _ = self._defender_dense(out, "out", n, partial=True)
        if n and out:
            _check(self.lib, self.lib.mcbs_unpack_defender_observation(self._h, packed.data_ptr(), _row_stride(packed, m), idx, m, n, C.byref(block),
                                                                       self._stream()), "mcbs_unpack_defender_observation")
        return out

    def encode_defender_features(self, dense: Optional[dict] = None, packed=None, index=None, out=None, dtype=None, bad_rows=None):
        """The float rows DefenderVecEnv.features() builds — the four fields as 0.0 / 1.0 in sorted key order, F = 13 N + S columns —
        in one launch (mcbs_encode_defender_features), from EITHER dense (the four int8 fields, m rows) OR packed (int32 [m, >= W_def]).
        index: optional device int64 [n]: output row i is built from source row index[i], read where it is stored; an index outside
        [0, m) reads nothing: that row is all zero and bad_rows (optional device int32 [1]) grows by one.  out: device float32 /
        bfloat16 / float16 [n, >= F] with contiguous rows (columns from F on are not touched, every column below is written), or None
        for a new tensor of `dtype` (default float32) whose rows are padded to whole 16-byte groups; returns the [n, F] view."""
        t = self.torch
        if (dense is None) == (packed is None):
            raise ValueError("exactly one of dense= and packed= is the source")
        if packed is not None:
            self._defender_packed_rows(packed, "packed")
            m, block, src, stride = packed.shape[0], None, packed.data_ptr(), _row_stride(packed, packed.shape[0])
        else:
            block, m = self._defender_dense(dense, "dense")
            block, src, stride = C.byref(block), None, 0
        idx, n = self._row_index(index, m)
        F = sum(self._defender_field_sizes().values())
        if out is None:
            dtype = dtype or t.float32
            if dtype not in self._feature_dtypes:
                raise ValueError("features dtype must be float32, bfloat16 or float16")
            per = 16 // self._feature_dtypes[dtype][1]
            out = t.empty((n, (F + per - 1) // per * per), dtype=dtype, device=self.device)
        if out.dtype not in self._feature_dtypes:
            raise ValueError("out must be float32, bfloat16 or float16")
        if dtype is not None and out.dtype != dtype:
            raise ValueError(f"out is {out.dtype}, dtype asks for {dtype}")
        self._rows(out, (out.dtype,), "out", n, F)
        if bad_rows is not None:
            self._counter(bad_rows, "bad_rows")
        if n:
            _check(self.lib, self.lib.mcbs_encode_defender_features(self._h, block, src, stride, idx, m, n, out.data_ptr(), _row_stride(out, n),
                                                                    self._feature_dtypes[out.dtype][0], _ptr(bad_rows), self._stream()),
                   "mcbs_encode_defender_features")
        return out[:, :F]

    def defender_wrapper_step_packed_launches(self) -> int:
        """Launches of one mcbs_defender_wrapper_step_packed of this batch: 1 (the turn writes the packed rows itself: up to 32 nodes),
        2, or 0 without a learned defender."""
        return int(self.lib.mcbs_defender_wrapper_step_packed_launches(self._h))

    def defender_wrapper_step_packed_call(self, packed, bufs, cfg):
        """callable(actions_ptr): mcbs_defender_wrapper_step_packed — the defender's wrapper step whose observation output is the packed
        row — with the argument blocks bound once.  packed: device int32 [E, >= W_def] with contiguous rows."""
        self._defender_packed_rows(packed, "packed", self.E)
        return self._bound("mcbs_defender_wrapper_step_packed", _ACTIONS, packed, _row_stride(packed, self.E), bufs, cfg, _STREAM)

    def get_state(self):
        rb = state_record_bytes(self.topo.n_nodes, self.spec.maximum_total_credentials)
        assert rb == self.lib.mcbs_state_record_bytes(self._h)
        buf = np.zeros(rb * self.E, np.uint8)
        _check(self.lib, self.lib.mcbs_get_state(self._h, buf.ctypes.data, buf.size), "mcbs_get_state")
        return split_state(buf, self.E, self.topo.n_nodes, self.spec.maximum_total_credentials)

    def set_state(self, hdr, nodes, order, cache) -> None:
        """Inverse of get_state (parity / debugging): upload canonical state records."""
        N, Cm = self.topo.n_nodes, self.spec.maximum_total_credentials
        rb = state_record_bytes(N, Cm)
        raw = np.zeros((self.E, rb), np.uint8)
        raw[:, :64] = np.ascontiguousarray(hdr.astype(STATE_HEADER_DT)).view(np.uint8).reshape(self.E, 64)
        raw[:, 64:64 + 32 * N] = np.ascontiguousarray(nodes.astype(STATE_NODE_DT)).view(np.uint8).reshape(self.E, 32 * N)
        o = 64 + 32 * N
        raw[:, o:o + 2 * N] = np.ascontiguousarray(order.astype("<u2")).view(np.uint8).reshape(self.E, 2 * N)
        raw[:, o + 2 * N:o + 2 * N + 2 * Cm] = np.ascontiguousarray(cache.astype("<u2")).view(np.uint8).reshape(self.E, 2 * Cm)
        _check(self.lib, self.lib.mcbs_set_state(self._h, raw.ctypes.data, raw.size), "mcbs_set_state")

    def variant(self) -> dict:
        """The compiled variant this batch dispatches to (mcbs_batch_variant): packed, words_per_set, wide, coop, lds_topo, defender_kind,
        fused_wrapper, fused_defender_obs.  Decided at creation; the query changes nothing."""
        v = BatchVariantInfo()
        _check(self.lib, self.lib.mcbs_batch_variant(self._h, C.byref(v)), "mcbs_batch_variant")
        return {name: int(getattr(v, name)) for name, _ in BatchVariantInfo._fields_}

    def step_is_lean(self, with_info: bool) -> bool:
        """Whether step(actions, with_info) of this batch takes the lean launch (packed, attacker-only batch, no info buffers)."""
        return bool(self.lib.mcbs_step_is_lean(self._h, int(bool(with_info))))

    def step_topo_traits(self, with_info: bool):
        """(narrow, traits): whether step(actions, with_info) of this batch takes the narrow lean kernel, and the MCBS_TOPO_* bits of the
        batch's topology (mcbs_step_topo_traits)."""
        t = C.c_uint32()
        narrow = self.lib.mcbs_step_topo_traits(self._h, int(bool(with_info)), C.byref(t))
        return bool(narrow), int(t.value)

    def timing_enable(self, on: bool = True) -> None:
        _check(self.lib, self.lib.mcbs_timing_enable(self._h, int(on)), "mcbs_timing_enable")

    def timing_read(self):
        ms, n = C.c_double(), C.c_uint64()
        _check(self.lib, self.lib.mcbs_timing_read(self._h, C.byref(ms), C.byref(n)), "mcbs_timing_read")
        return ms.value, n.value
