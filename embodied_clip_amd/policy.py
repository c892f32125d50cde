"""Drop-in ``ResnetTensorObjectNavActorCritic`` (an AllenAct ``ActorCriticModel``)
whose forward AND backward are the hand-written gfx950 kernels behind
``ec_policy_forward`` / ``ec_policy_backward`` (include/ec_amd.h).

Mirrors [U] allenai/allenact ~v0.5.0
``projects/objectnav_baselines/models/object_nav_models.py`` (the model the
reference's RoboTHOR config instantiates:
readme_files/baselines_robothor_objectnav.md:51) -- same constructor keywords,
``forward(observations, memory, prev_actions, masks)`` contract, recurrent
memory specification and parameter names, so checkpoints,
optimisers and the engine's per-parameter all-reduce keep working.

MI355X-first differences, invisible through the API:
  * all 17 parameters are views into ONE flat fp32 buffer (and their grads into
    one flat grad buffer): a single RCCL all-reduce bucket and one fused
    clip+Adam launch instead of 17 of each;
  * the forward is autograd-visible through a ``torch.autograd.Function`` whose
    backward is the HIP backward (no torch autograd graph inside the policy).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, spaces
from .synthetic import POLICY_PARAM_ORDER, policy_param_order, policy_param_shapes


# ---- AllenAct base abstractions (the real ones when allenact is importable) ----------------------
from .allenact_compat import ActorCriticModel, ActorCriticOutput, CategoricalDistr, Memory  # noqa: E402,F401


# ---- handle ----------------------------------------------------------------------------------

class PolicyHandle:
    """``ec_policy_t`` plus the flat-buffer layout."""

    def __init__(self, rnn_type: str = "GRU", rnn_layers: int = 1, **cfg: int):
        """``rnn_layers = L`` (1..4; torch's ``num_layers``): the state row is layer-major, ``[h^0 | h^1 | ...]`` or
        ``[h^0 | c^0 | h^1 | c^1 | ...]``, of width ``state_width == L * SW`` (``memory_to_state`` / ``state_to_memory`` convert
        upstream's memory); the upper layers' tensors end ``param_order``.  ``rnn_type``: "GRU" (the default: ``ec_policy_create``'s handle exactly) or "LSTM" -- the recurrent state of an
        actor is then one row ``[h | c]`` of width ``state_width == 2 * hidden``, which is what ``h0`` / ``h_final`` /
        ``dh_final`` of every method below hold."""
        self.lib = _lib.load()
        self.rnn_type, self.rnn_layers = self._check_rnn(rnn_type, rnn_layers)
        self.cfg = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6,
                        compress_hid=128, compress_out=32, comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0,
                        prev_action_dims=0, prev_action_null=0)
        self.cfg.update(cfg)
        self.goal_in = self.cfg["goal_in"]      # > 0: the goal of a frame is goal_in floats (PointNav), ec_policy_*_vec
        # > 0: the previous action's embedding (this wide) is concatenated to the GRU input; ec_policy_forward_pa / ec_policy_act_pa
        self.prev_action_dims = self.cfg["prev_action_dims"]
        if rnn_layers > 1 and (self.cfg["dual"] or self.cfg["fusion"]):
            raise ValueError("the two-tower and zero-shot agents keep one recurrent layer")
        self.param_order = policy_param_order(self.cfg["dual"], self.goal_in, self.prev_action_dims, self.cfg["prev_action_null"],
                                              rnn_layers=rnn_layers)
        c = _lib.PolicyCfg(**self.cfg)
        h = C.c_void_p()
        _lib.check(self.lib.ec_policy_create_rnn_layers(C.byref(h), C.byref(c), _lib.RNN_TYPES[rnn_type], rnn_layers),
                   "ec_policy_create_rnn_layers")
        self._bind_layout(h, policy_param_shapes(**self.cfg, rnn_type=rnn_type, rnn_layers=rnn_layers), self.param_order)

    @staticmethod
    def _check_rnn(rnn_type, rnn_layers):
        """The recurrent arguments of every handle constructor.  -> (rnn_type, rnn_layers)"""
        if rnn_type not in _lib.RNN_TYPES:
            raise ValueError(f"rnn_type must be one of {sorted(_lib.RNN_TYPES)}, got {rnn_type!r}")
        if not (isinstance(rnn_layers, int) and 1 <= rnn_layers <= 4):
            raise ValueError(f"rnn_layers must be 1..4, got {rnn_layers!r}")
        return rnn_type, rnn_layers

    def _bind_layout(self, h, shapes, param_order=None) -> None:
        """Adopt the created ``ec_policy_t`` and read its flat layout: ``flat_size``, ``state_width`` (L * (H, or 2H on an LSTM
        handle)) and every tensor's (offset, elements), checked against ``shapes`` (name -> shape, in flat order)."""
        self.h = h
        self.flat_size = self.lib.ec_policy_flat_size(h)
        self.state_width = self.lib.ec_policy_state_width(h)
        self.shapes = shapes
        self.param_order = tuple(shapes) if param_order is None else param_order
        self.offsets: "OrderedDict[str, Tuple[int, int]]" = OrderedDict()
        assert self.lib.ec_policy_num_param_tensors(h) == len(self.param_order)
        for i, name in enumerate(self.param_order):
            off, num = C.c_size_t(), C.c_size_t()
            _lib.check(self.lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)))
            n = 1
            for d in self.shapes[name]:
                n *= d
            assert n == num.value, (name, n, num.value)
            self.offsets[name] = (off.value, num.value)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ec_policy_destroy(self.h)
                self.h = None
        except Exception:
            pass

    _net_name = None        # ("pooled" / "two-view" on the handles of the nets that have no goal table)

    def set_goal_table(self, table: torch.Tensor) -> None:
        """``fusion=1``: frozen goal table f32 [num_goals, in_channels] (CLIP text embeddings of the goal prompts)."""
        if self._net_name:
            raise ValueError(f"the {self._net_name} net has no goal table")
        assert table.dtype == torch.float32 and table.is_contiguous()
        assert tuple(table.shape) == (self.cfg["num_goals"], self.cfg["in_channels"]), table.shape
        self._goal_table = table          # the handle borrows the pointer: keep the tensor alive
        _lib.check(self.lib.ec_policy_set_goal_table(self.h, table.data_ptr()), "ec_policy_set_goal_table")

    @property
    def A(self):
        return self.cfg["num_actions"]

    @property
    def H(self):
        return self.cfg["hidden"]

    def _goal_ptr(self, goal, rows: int) -> int:
        """The goal argument of the handle's entry points: int64 ids [rows], or (``goal_in > 0``) float32 [rows, goal_in]."""
        if self.goal_in:
            assert goal.dtype == torch.float32 and goal.is_contiguous() and tuple(goal.shape) == (rows, self.goal_in), \
                (goal.dtype, tuple(goal.shape), (rows, self.goal_in))
        else:
            assert goal.dtype == torch.int64 and goal.numel() == rows, (goal.dtype, tuple(goal.shape))
        return goal.data_ptr()

    def _state_ptr(self, t, N: int, what: str) -> int:
        """A recurrent-state argument (``h0`` / ``h_final`` / ``dh_final``): f32 ``[N, state_width]``, contiguous."""
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N * self.state_width, \
            (what, t.dtype, tuple(t.shape), (N, self.state_width))
        return t.data_ptr()

    def _prev_ptr(self, prev_actions, rows: int) -> int:
        """The previous actions of the ``_pa`` entry points: int64 [rows] on a handle with the embedding, None without."""
        if not self.prev_action_dims:
            assert prev_actions is None, "this handle has no previous-action embedding (prev_action_dims=0): pass prev_actions=None"
            return 0
        assert prev_actions is not None, "a handle with prev_action_dims > 0 needs prev_actions (int64, one per frame)"
        assert prev_actions.dtype == torch.int64 and prev_actions.is_contiguous() and prev_actions.numel() == rows, \
            (prev_actions.dtype, tuple(prev_actions.shape), rows)
        return prev_actions.data_ptr()

    def _outputs(self, hv, h_final, T: int, N: int, dev):
        """``hv`` [T*N, A+1] and ``h_final`` [N, state_width] of a forward: the caller's, or fresh ones on ``dev``."""
        if hv is None:
            hv = torch.empty((T * N, self.A + 1), dtype=torch.float32, device=dev)
        if h_final is None:
            h_final = torch.empty((N, self.state_width), dtype=torch.float32, device=dev)
        return hv, h_final

    # ---- the one forward and the one act path.  A call's arguments are: the handle and the parameters; the leading pointers of
    # the handle's face (``_face``, the one hook a subclass supplies); the state block; for an act call the outputs and the
    # selection block; the stream.

    def _face(self, kind: str, feat, goal, feat2, prev_actions, sensors, rows: int, deterministic: bool = False):
        """Check the inputs of a call over ``rows`` frames; -> (entry-point name, the pointers between ``params`` and ``h0``).
        ``kind``: "forward", "act" (the narrow act entry points: a handle without previous actions) or "act_ex"."""
        assert feat.is_contiguous() and feat.dtype in (torch.bfloat16, torch.float32)
        assert sensors is None, "this handle has no sensors: pass sensors=None"
        if kind == "forward" and self.cfg["dual"]:    # RGB + depth: feat = the RGB features, feat2 = the depth features (same shape / dtype)
            assert feat2 is not None and feat2.is_contiguous() and feat2.dtype == feat.dtype and feat2.shape == feat.shape
        fp, f2, bf = feat.data_ptr(), _lib.ptr(feat2), int(feat.dtype == torch.bfloat16)
        pp, gp = self._prev_ptr(prev_actions, rows), self._goal_ptr(goal, rows)
        if kind == "act":
            return ("ec_policy_act_vec" if self.goal_in else "ec_policy_act") + ("_greedy" if deterministic else ""), (fp, f2, bf, gp)
        if kind == "forward" and not pp:
            return ("ec_policy_forward_vec" if self.goal_in else "ec_policy_forward2"), (fp, f2, bf, gp)
        ids, vec = (0, gp) if self.goal_in else (gp, 0)      # these entry points take the ids and the coordinates
        if pp:
            return ("ec_policy_forward_pa" if kind == "forward" else "ec_policy_act_pa"), (fp, f2, bf, ids, vec, pp)
        return "ec_policy_act_ex", (fp, f2, bf, ids, vec)

    def _state_block(self, h0, masks, sizes, ws, flag, hv, h_final):
        """State in, masks, ``sizes`` ((T, N) of a forward, (N,) of an act call), workspace, the mode flag, ``hv`` and state out."""
        N = sizes[-1]
        return (self._state_ptr(h0, N, "h0"), masks.data_ptr(), *sizes, ws.data_ptr(), ws.numel() * ws.element_size(), int(flag),
                hv.data_ptr(), self._state_ptr(h_final, N, "h_final"))

    @staticmethod
    def _select_block(deterministic, seed, step, first_actor, expert_actions, expert_mask, force_p: float):
        """The selection arguments of the one-call act entry points, ending in the teacher-forcing triple (zeros: no forcing)."""
        if expert_actions is not None and force_p > 0.0:
            return int(deterministic), seed, step, first_actor, expert_actions.data_ptr(), expert_mask.data_ptr(), force_p
        return int(deterministic), seed, step, first_actor, 0, 0, 0.0

    def _call(self, name: str, flat_params, *args):
        with _lib.tensor_guard(flat_params):
            _lib.check(getattr(self.lib, name)(self.h, flat_params.data_ptr(), *args, _lib.stream_ptr()), name)

    def memory_to_state(self, mem: torch.Tensor) -> torch.Tensor:
        return memory_to_state(mem, self.rnn_type, self.rnn_layers)

    def state_to_memory(self, state: torch.Tensor) -> torch.Tensor:
        return state_to_memory(state, self.rnn_type, self.rnn_layers)

    def workspace_bytes(self, T: int, N: int, backward: bool) -> int:
        return self.lib.ec_policy_workspace_bytes(self.h, T, N, int(backward))

    def flatten(self, sd: Dict[str, torch.Tensor], device) -> torch.Tensor:
        flat = torch.zeros(self.flat_size, dtype=torch.float32, device=device)
        for name, (off, num) in self.offsets.items():
            flat[off:off + num].copy_(sd[name].reshape(-1).to(device=device, dtype=torch.float32))
        return flat

    def views(self, flat: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((n, flat[o:o + k].view(self.shapes[n])) for n, (o, k) in self.offsets.items())

    def forward(self, flat_params, feat, goal, h0, masks, T, N, ws, hv=None, h_final=None, for_backward: bool = True,
                reuse_tables: bool = False, feat2=None, prev_actions=None, sensors=None):
        """feat: bf16 or fp32 NHWC rows [T*N, S*S, C]; returns (hv [T*N, A+1], h_final [N, state_width]).
        ``for_backward=True`` (default) keeps every activation ``backward`` needs and wants a workspace of
        ``workspace_bytes(T, N, True)``; ``False`` is the inference-only act step (``workspace_bytes(T, N, False)``).
        The kernel plan follows this flag, never the size of ``ws``.  ``reuse_tables`` (inference only): the weight-derived
        tables a previous ``for_backward=False`` call left in THIS ``ws`` are still valid (same parameters: the later act
        steps of a rollout).  ``prev_actions`` (handles with ``prev_action_dims > 0``, and only those): int64 [T*N], row
        ``t * N + n`` = the action actor ``n`` took at step ``t - 1``.  ``sensors`` (the pooled net's handle, and only that one): f32
        ``[T*N, K]``; None on every other handle."""
        mode = 1 if for_backward else (2 if reuse_tables else 0)
        hv, h_final = self._outputs(hv, h_final, T, N, flat_params.device)
        name, lead = self._face("forward", feat, goal, feat2, prev_actions, sensors, T * N)
        self._call(name, flat_params, *lead, *self._state_block(h0, masks, (T, N), ws, mode, hv, h_final))
        return hv, h_final

    def act(self, flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed: int = 0, step: int = 0,
            first_actor: int = 0, reuse_tables: bool = False, feat2=None, deterministic: bool = False, prev_actions=None, sensors=None):
        """The act step in one call (``ec_policy_act``): the T = 1 inference forward whose heads launch also samples
        ``actions`` / ``logp`` (and copies ``values``) -- the results of ``forward(for_backward=False)`` + ``ec_sample_actions``.
        ``deterministic=True`` (evaluation): the heads launch takes ``CategoricalDistr.mode()`` instead, the first maximal logit
        (``ec_policy_act_greedy``; ``seed`` / ``step`` / ``first_actor`` are not used) -- ``forward`` + ``ec_mode_actions``."""
        if self.prev_action_dims:            # (one entry point serves every act step of such a handle)
            return self.act_ex(flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed, step, first_actor,
                               reuse_tables, feat2, deterministic, prev_actions=prev_actions, sensors=sensors)
        name, lead = self._face("act", feat, goal, feat2, prev_actions, sensors, N, deterministic)
        self._call(name, flat_params, *lead, *self._state_block(h0, masks, (N,), ws, reuse_tables, hv, h_final),
                   actions.data_ptr(), logp.data_ptr(), _lib.ptr(values), *(() if deterministic else (seed, step, first_actor)))
        return hv, h_final

    def act_ex(self, flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed: int = 0, step: int = 0,
               first_actor: int = 0, reuse_tables: bool = False, feat2=None, deterministic: bool = False, expert_actions=None,
               expert_mask=None, force_p: float = 0.0, prev_actions=None, sensors=None):
        """The act step in one call for every handle, up to 256 actions (``ec_policy_act_ex``).  With more than 7 actions the
        heads launch of the wide action space computes the logits and selects (sample, or ``deterministic=True`` the first
        maximal logit) -- the results of ``forward(for_backward=False)`` + ``ec_sample_actions`` / ``ec_mode_actions`` on the
        ``hv`` it writes, bit for bit; with up to 7 it is ``act``.  ``expert_actions`` / ``expert_mask`` / ``force_p``: teacher
        forcing (``imitation.teacher_force``) in the same call -- inside the heads launch of a wide action space."""
        name, lead = self._face("act_ex", feat, goal, feat2, prev_actions, sensors, N)
        self._call(name, flat_params, *lead, *self._state_block(h0, masks, (N,), ws, reuse_tables, hv, h_final),
                   actions.data_ptr(), logp.data_ptr(), _lib.ptr(values),
                   *self._select_block(deterministic, seed, step, first_actor, expert_actions, expert_mask, force_p))
        return hv, h_final

    def backward(self, flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, feat2=None, recurrent_ready=None):
        """``recurrent_ready``: a ``torch.cuda.Event`` (already recorded once, so that its handle exists) the library records
        on the current stream when ``flat_grads[self.recurrent_section()]`` is final (``ec_policy_backward3``)."""
        with _lib.tensor_guard(flat_params):
            return self._backward(flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, feat2, recurrent_ready)

    def _backward(self, flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, feat2=None, recurrent_ready=None):
        if self.cfg["dual"]:
            assert feat2 is not None and feat2.is_contiguous() and feat2.dtype == feat.dtype and feat2.shape == feat.shape
        if dh_final is not None:
            self._state_ptr(dh_final, N, "dh_final")
        ev = None
        if recurrent_ready is not None:
            ev = int(recurrent_ready.cuda_event)
            assert ev, "record the event once before handing it over (torch creates the hipEvent_t lazily)"
        _lib.check(self.lib.ec_policy_backward3(
            self.h, flat_params.data_ptr(), feat.data_ptr(), _lib.ptr(feat2), int(feat.dtype == torch.bfloat16), masks.data_ptr(),
            T, N, ws.data_ptr(), ws.numel() * ws.element_size(), dhv.data_ptr(), _lib.ptr(dh_final), flat_grads.data_ptr(),
            ev, _lib.stream_ptr()), "ec_policy_backward3")
        return flat_grads

    def recurrent_section(self) -> slice:
        """The contiguous part of the flat bucket whose gradients ``ec_policy_backward3`` finishes first (GRU + both heads:
        ``state_encoder.rnn.weight_ih_l0`` ... ``critic.fc.bias``); the rest is the goal encoder's."""
        o0 = self.offsets["state_encoder.rnn.weight_ih_l0"][0]
        o1, k1 = self.offsets["critic.fc.bias"]
        end = o1 + k1
        later = [o for (o, _) in self.offsets.values() if o >= end]      # (the dual encoder's depth stream; upper recurrent layers)
        return slice(o0, min(later) if later else self.flat_size)


# ---- the pooled-embedding net ------------------------------------------------------------------
# [U] habitat-lab ``PointNavResNetNet`` (habitat_baselines/rl/ddppo/policy/resnet_policy.py) over ONE pooled CLIP vector per frame,
# the Habitat DD-PPO branch of readme_files/baselines_habitat.md.  Restated from the published sources, which are not under the
# reference tree: parity unpinned.  The ONE table of tensor names (Habitat's, without the ``net.`` prefix) in flat order:
POOLED_SENSOR_NAMES = {(3,): ("tgt_embeding",), (2, 2): ("gps_embedding", "compass_embedding")}   # (sic: upstream's spelling)
POOLED_EMBEDDING_TENSORS = ("obj_categories_embedding.weight", "prev_action_embedding.weight")    # nn.Embedding: N(0, 1)


def pooled_sensor_names(sensors) -> Tuple[str, ...]:
    """Habitat's module names for the usual sensor sets (PointNav's 3-float goal; ObjectNav's GPS + compass), else by position."""
    sensors = tuple(int(k) for k in sensors)
    return POOLED_SENSOR_NAMES.get(sensors, tuple(f"sensor{i}_embedding" for i in range(len(sensors))))


def pooled_param_shapes(embed_in: int, hidden: int = 512, num_goals: int = 12, sensors=(), num_actions: int = 6,
                        prev_action_dims: int = 0, prev_action_null: int = 1, rnn_type: str = "GRU", rnn_layers: int = 1,
                        embed_dims: int = 32) -> "OrderedDict[str, Tuple[int, ...]]":
    """Tensor name -> shape in the flat order of ``ec_policy_create_pooled``.  ``weight_ih_l0``'s columns: ``v`` (hidden), the
    goal-id embedding, the sensors in order, the previous action."""
    sensors = tuple(int(k) for k in sensors)
    G = (4 if rnn_type == "LSTM" else 3) * hidden
    ids = 1 if num_goals > 0 else 0
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    out["visual_fc.1.weight"] = (hidden, embed_in)
    out["visual_fc.1.bias"] = (hidden,)
    if ids:
        out["obj_categories_embedding.weight"] = (num_goals, embed_dims)
    for name, k in zip(pooled_sensor_names(sensors), sensors):
        out[f"{name}.weight"] = (embed_dims, k)
        out[f"{name}.bias"] = (embed_dims,)
    out["state_encoder.rnn.weight_ih_l0"] = (G, hidden + embed_dims * (ids + len(sensors)) + prev_action_dims)
    out["state_encoder.rnn.weight_hh_l0"] = (G, hidden)
    out["state_encoder.rnn.bias_ih_l0"] = (G,)
    out["state_encoder.rnn.bias_hh_l0"] = (G,)
    out["action_distribution.linear.weight"] = (num_actions, hidden)
    out["action_distribution.linear.bias"] = (num_actions,)
    out["critic.fc.weight"] = (1, hidden)
    out["critic.fc.bias"] = (1,)
    if prev_action_dims:
        out["prev_action_embedding.weight"] = (num_actions + prev_action_null, prev_action_dims)
    for l in range(1, rnn_layers):
        out[f"state_encoder.rnn.weight_ih_l{l}"] = (G, hidden)
        out[f"state_encoder.rnn.weight_hh_l{l}"] = (G, hidden)
        out[f"state_encoder.rnn.bias_ih_l{l}"] = (G,)
        out[f"state_encoder.rnn.bias_hh_l{l}"] = (G,)
    return out


class PooledPolicyHandle(PolicyHandle):
    """``ec_policy_create_pooled``'s handle (``PolicyHandle.pooled``): ``forward`` / ``act`` take the embedding rows f32 ``[T*N, D]`` as
    ``feat`` and ``goal=`` (int64 ids, handles with ``num_goals > 0``), ``sensors=`` (f32 ``[T*N, K]``, handles with sensors),
    ``prev_actions=``; ``backward``, ``flatten``, ``views``, ``recurrent_section`` are the base class's."""
    _net_name = "pooled"

    def __init__(self, embed_in: int, hidden: int = 512, num_goals: int = 12, sensors=(), num_actions: int = 6,
                 prev_action_dims: int = 0, prev_action_null: int = 1, rnn_type: str = "GRU", rnn_layers: int = 1, embed_dims: int = 32):
        self.lib = _lib.load()
        self.rnn_type, self.rnn_layers = self._check_rnn(rnn_type, rnn_layers)
        sensors = tuple(int(k) for k in sensors)
        if len(sensors) > 3 or any(k < 1 for k in sensors) or sum(sensors) > 8:
            raise ValueError(f"at most 3 sensors of at least one float each, 8 floats in all, got {sensors!r}")
        if not num_goals and not sensors:
            raise ValueError("the pooled net needs a goal: num_goals > 0 or at least one sensor")
        if not prev_action_dims:
            prev_action_null = 0
        self.sensors, self.K = sensors, sum(sensors)
        self.pooled_cfg = dict(embed_in=embed_in, hidden=hidden, num_goals=num_goals, sensors=sensors, num_actions=num_actions,
                               prev_action_dims=prev_action_dims, prev_action_null=prev_action_null, rnn_type=rnn_type,
                               rnn_layers=rnn_layers, embed_dims=embed_dims)
        self.cfg = dict(hidden=hidden, num_goals=num_goals, num_actions=num_actions, prev_action_dims=prev_action_dims,
                        prev_action_null=prev_action_null, dual=0, fusion=0, goal_in=0, embed_in=embed_in)
        self.goal_in = 0
        self.prev_action_dims = prev_action_dims
        c = _lib.PooledCfg(embed_in=embed_in, hidden=hidden, embed_dims=embed_dims, num_goals=num_goals, num_sensors=len(sensors),
                           sensor_in=(C.c_int * 3)(*(sensors + (0,) * (3 - len(sensors)))), num_actions=num_actions,
                           prev_action_dims=prev_action_dims, prev_action_null=prev_action_null, rnn_type=_lib.RNN_TYPES[rnn_type],
                           num_layers=rnn_layers)
        h = C.c_void_p()
        _lib.check(self.lib.ec_policy_create_pooled(C.byref(h), C.byref(c)), "ec_policy_create_pooled")
        self._bind_layout(h, pooled_param_shapes(**self.pooled_cfg))

    def _face(self, kind: str, feat, goal, feat2, prev_actions, sensors, rows: int, deterministic: bool = False):
        assert feat2 is None
        D = self.pooled_cfg["embed_in"]
        assert feat.dtype == torch.float32 and feat.is_contiguous() and feat.numel() == rows * D, (feat.dtype, tuple(feat.shape), (rows, D))
        if self.pooled_cfg["num_goals"]:
            assert goal is not None and goal.dtype == torch.int64 and goal.is_contiguous() and goal.numel() == rows, "goal: int64, one id per frame"
        else:
            assert goal is None, "this handle has no goal-id embedding (num_goals=0): pass goal=None"
        if self.K:
            assert sensors is not None and sensors.dtype == torch.float32 and sensors.is_contiguous() and sensors.numel() == rows * self.K, \
                f"sensors: float32 [{rows}, {self.K}]"
        else:
            assert sensors is None, "this handle has no sensors: pass sensors=None"
        name = "ec_policy_forward_pooled" if kind == "forward" else "ec_policy_act_pooled"
        return name, (feat.data_ptr(), _lib.ptr(goal), _lib.ptr(sensors), self._prev_ptr(prev_actions, rows))

    def act(self, flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed: int = 0, step: int = 0,
            first_actor: int = 0, reuse_tables: bool = False, feat2=None, deterministic: bool = False, prev_actions=None, sensors=None,
            expert_actions=None, expert_mask=None, force_p: float = 0.0):
        """``ec_policy_act_pooled``: the T = 1 inference forward and the selection (sample, ``deterministic=True`` the first maximal
        logit, optional teacher forcing) in one call, 2..256 actions."""
        return PolicyHandle.act_ex(self, flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed, step, first_actor,
                                   reuse_tables, feat2, deterministic, expert_actions, expert_mask, force_p, prev_actions, sensors)

    act_ex = act

    def _backward(self, flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, feat2=None, recurrent_ready=None):
        assert feat.dtype == torch.float32 and feat.is_contiguous()
        return super()._backward(flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, None, recurrent_ready)


def _pooled(embed_in: int, hidden: int = 512, num_goals: int = 12, sensors=(), num_actions: int = 6, prev_action_dims: int = 0,
            prev_action_null: int = 1, rnn_type: str = "GRU", rnn_layers: int = 1) -> PooledPolicyHandle:
    """``PolicyHandle.pooled(...)``: the handle of the pooled-embedding net (``PooledPolicyHandle``)."""
    return PooledPolicyHandle(embed_in, hidden, num_goals, sensors, num_actions, prev_action_dims, prev_action_null, rnn_type, rnn_layers)


PolicyHandle.pooled = staticmethod(_pooled)


# ---- the two-view rearrangement net --------------------------------------------------------------
# [U] ai2thor-rearrangement ``ResNetRearrangeActorCriticRNN`` (the 1-Phase Embodied CLIP ResNet50 IL agent of
# readme_files/baselines_ithor_rearrangement.md) over TWO frozen CLIP maps per frame: the current view and the goal-state view.
# Restated from the published sources, which are not under the reference tree: parity unpinned.  The ONE table of tensor names in
# flat order; the three convs keep upstream's 4-D ``nn.Conv2d`` shapes, so an upstream state dict flattens unchanged.
TWO_VIEW_PREV_ACTION_EMBEDDER = "prev_action_embedder.weight"     # nn.Embedding(A + 1, E); upstream E = hidden


def two_view_param_shapes(in_channels: int = 2048, hidden: int = 512, num_actions: int = 84, attn_hidden: int = 32,
                          prev_action_dims: int = 0, prev_action_null: int = 1, rnn_type: str = "LSTM", rnn_layers: int = 1,
                          spatial: int = 7) -> "OrderedDict[str, Tuple[int, ...]]":
    """Tensor name -> shape in the flat order of ``ec_policy_create_two_view``.  ``weight_ih_l0``'s columns: ``v`` (hidden), then
    the previous action's embedding."""
    G = (4 if rnn_type == "LSTM" else 3) * hidden
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    out["visual_encoder.0.weight"] = (hidden, 3 * in_channels, 1, 1)
    out["visual_encoder.0.bias"] = (hidden,)
    out["visual_attention.0.weight"] = (attn_hidden, 3 * in_channels, 1, 1)
    out["visual_attention.0.bias"] = (attn_hidden,)
    out["visual_attention.2.weight"] = (1, attn_hidden, 1, 1)
    out["visual_attention.2.bias"] = (1,)
    out["state_encoder.rnn.weight_ih_l0"] = (G, hidden + prev_action_dims)
    out["state_encoder.rnn.weight_hh_l0"] = (G, hidden)
    out["state_encoder.rnn.bias_ih_l0"] = (G,)
    out["state_encoder.rnn.bias_hh_l0"] = (G,)
    out["actor.linear.weight"] = (num_actions, hidden)
    out["actor.linear.bias"] = (num_actions,)
    out["critic.fc.weight"] = (1, hidden)
    out["critic.fc.bias"] = (1,)
    if prev_action_dims:
        out[TWO_VIEW_PREV_ACTION_EMBEDDER] = (num_actions + prev_action_null, prev_action_dims)
    for l in range(1, rnn_layers):
        out[f"state_encoder.rnn.weight_ih_l{l}"] = (G, hidden)
        out[f"state_encoder.rnn.weight_hh_l{l}"] = (G, hidden)
        out[f"state_encoder.rnn.bias_ih_l{l}"] = (G,)
        out[f"state_encoder.rnn.bias_hh_l{l}"] = (G,)
    return out


class TwoViewPolicyHandle(PolicyHandle):
    """``ec_policy_create_two_view``'s handle (``PolicyHandle.two_view``): ``forward`` / ``act`` / ``backward`` take the current
    view's features as ``feat`` and the goal view's as ``feat2``, both bf16 ``[T*N, S2, C]``, and ``prev_actions=``; ``goal`` is
    None.  ``flatten``, ``views``, ``recurrent_section`` are the base class's."""
    _net_name = "two-view"

    def __init__(self, in_channels: int, hidden: int = 512, num_actions: int = 84, attn_hidden: int = 32, prev_action_dims: int = 0,
                 prev_action_null: int = 1, rnn_type: str = "LSTM", rnn_layers: int = 1, spatial: int = 7):
        self.lib = _lib.load()
        self.rnn_type, self.rnn_layers = self._check_rnn(rnn_type, rnn_layers)
        if not prev_action_dims:
            prev_action_null = 0
        self.two_view_cfg = dict(in_channels=in_channels, hidden=hidden, num_actions=num_actions, attn_hidden=attn_hidden,
                                 prev_action_dims=prev_action_dims, prev_action_null=prev_action_null, rnn_type=rnn_type,
                                 rnn_layers=rnn_layers, spatial=spatial)
        self.cfg = dict(hidden=hidden, num_goals=0, num_actions=num_actions, prev_action_dims=prev_action_dims,
                        prev_action_null=prev_action_null, dual=0, fusion=0, goal_in=0, in_channels=in_channels, spatial=spatial)
        self.goal_in = 0
        self.prev_action_dims = prev_action_dims
        c = _lib.TwoViewCfg(in_channels=in_channels, spatial=spatial, hidden=hidden, attn_hidden=attn_hidden, num_actions=num_actions,
                            prev_action_dims=prev_action_dims, prev_action_null=prev_action_null, rnn_type=_lib.RNN_TYPES[rnn_type],
                            num_layers=rnn_layers)
        h = C.c_void_p()
        _lib.check(self.lib.ec_policy_create_two_view(C.byref(h), C.byref(c)), "ec_policy_create_two_view")
        self._bind_layout(h, two_view_param_shapes(**self.two_view_cfg))

    def _face(self, kind: str, feat, goal, feat2, prev_actions, sensors, rows: int, deterministic: bool = False):
        assert sensors is None, "this handle has no sensors: pass sensors=None"
        n = rows * self.cfg["spatial"] ** 2 * self.cfg["in_channels"]
        assert goal is None, "the two-view net has no goal input: pass goal=None"
        for t in (feat, feat2):
            assert t is not None and t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() == n, \
                "feat (current view) and feat2 (goal view): bf16 [rows, S2, C]"
        name = "ec_policy_forward_two_view" if kind == "forward" else "ec_policy_act_two_view"
        return name, (feat.data_ptr(), feat2.data_ptr(), self._prev_ptr(prev_actions, rows))

    def act(self, flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed: int = 0, step: int = 0,
            first_actor: int = 0, reuse_tables: bool = False, feat2=None, deterministic: bool = False, prev_actions=None,
            expert_actions=None, expert_mask=None, force_p: float = 0.0, sensors=None):
        """``ec_policy_act_two_view``: the T = 1 inference forward and the selection (sample, ``deterministic=True`` the first maximal
        logit, optional teacher forcing) in one call, 2..256 actions."""
        return PolicyHandle.act_ex(self, flat_params, feat, goal, h0, masks, N, ws, hv, h_final, actions, logp, values, seed, step, first_actor,
                                   reuse_tables, feat2, deterministic, expert_actions, expert_mask, force_p, prev_actions, sensors)

    act_ex = act

    def _backward(self, flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, feat2=None, recurrent_ready=None):
        for t in (feat, feat2):
            assert t is not None and t.dtype == torch.bfloat16 and t.is_contiguous(), "feat and feat2: the two views' bf16 features"
        return super()._backward(flat_params, feat, masks, T, N, ws, dhv, dh_final, flat_grads, feat2, recurrent_ready)


def _two_view(in_channels: int, hidden: int = 512, num_actions: int = 84, attn_hidden: int = 32, prev_action_dims: int = 0,
              prev_action_null: int = 1, rnn_type: str = "LSTM", rnn_layers: int = 1, spatial: int = 7) -> TwoViewPolicyHandle:
    """``PolicyHandle.two_view(...)``: the handle of the two-view rearrangement net (``TwoViewPolicyHandle``)."""
    return TwoViewPolicyHandle(in_channels, hidden, num_actions, attn_hidden, prev_action_dims, prev_action_null, rnn_type, rnn_layers,
                               spatial)


PolicyHandle.two_view = staticmethod(_two_view)


def memory_to_state(mem: torch.Tensor, rnn_type: str = "GRU", rnn_layers: int = 1) -> torch.Tensor:
    """Upstream's recurrent memory -> the handle's state rows.  ``mem``: ``[L, N, H]`` (GRU) or ``[2L, N, H]`` (LSTM: all ``h``
    layers, then all ``c`` layers -- ``torch.cat([h, c], 0)``, [U] RNNStateEncoder).  Returns ``[N, L * SW]``, layer-major:
    ``[h^0 | h^1 | ...]`` or ``[h^0 | c^0 | h^1 | c^1 | ...]``."""
    L = rnn_layers
    k = 2 if rnn_type == "LSTM" else 1
    if rnn_type not in _lib.RNN_TYPES or mem.dim() != 3 or mem.shape[0] != k * L:
        raise ValueError(f"memory of a {L}-layer {rnn_type} is [{k * L}, N, H], got {tuple(mem.shape)}")
    _, N, H = mem.shape
    # [k, L, N, H] -> [N, L, k, H]
    return mem.reshape(k, L, N, H).permute(2, 1, 0, 3).reshape(N, L * k * H).contiguous()


def state_to_memory(state: torch.Tensor, rnn_type: str = "GRU", rnn_layers: int = 1) -> torch.Tensor:
    """The inverse of ``memory_to_state``: ``[N, L * SW]`` rows -> ``[L, N, H]`` / ``[2L, N, H]``."""
    L = rnn_layers
    k = 2 if rnn_type == "LSTM" else 1
    if rnn_type not in _lib.RNN_TYPES or state.dim() != 2 or state.shape[1] % (k * L):
        raise ValueError(f"state rows of a {L}-layer {rnn_type} are [N, {k * L} * H], got {tuple(state.shape)}")
    N, H = state.shape[0], state.shape[1] // (k * L)
    return state.reshape(N, L, k, H).permute(2, 1, 0, 3).reshape(k * L, N, H).contiguous()


class _PolicyFn(torch.autograd.Function):
    """Autograd bridge: HIP forward, HIP backward.  ``owner`` (the nn.Module, or None) lends a scratch gradient
    bucket.  Workspaces come from torch's caching allocator, one per forward: a learn workspace lives exactly as long
    as the autograd node that saved it (so ``retain_graph`` / two live forwards can never share one), an act workspace
    dies with the call; reuse is the allocator's, stream-ordered.  Whether the forward keeps the activations of a
    backward is stated explicitly (``for_backward=need_grad``), so an act step always takes the act-step kernel plan."""

    @staticmethod
    def forward(ctx, handle: PolicyHandle, owner, flat, feat, feat2, goal, prev_actions, h0, masks, T, N, *params):
        need_grad = any(ctx.needs_input_grad)   # (grad mode is always off inside Function.forward)
        ws = torch.empty(handle.workspace_bytes(T, N, need_grad), dtype=torch.uint8, device=flat.device)
        hv, h_final = handle.forward(flat, feat, goal, h0, masks, T, N, ws, for_backward=need_grad, feat2=feat2,
                                     prev_actions=prev_actions)       # (a learn pass leaves the indices in ws for the backward)
        if need_grad:
            ctx.handle, ctx.owner, ctx.T, ctx.N = handle, owner, T, N
            ctx.feat2 = feat2                    # (the depth stream's features of the dual encoder, or None: frozen input)
            ctx.save_for_backward(flat, feat, masks, ws)
        return hv, h_final

    @staticmethod
    def backward(ctx, dhv, dh_final):
        flat, feat, masks, ws = ctx.saved_tensors
        h: PolicyHandle = ctx.handle
        owner = ctx.owner
        # the scratch bucket may only be lent when every .grad is already bound (autograd then accumulates INTO the
        # bound views and never keeps a reference to what is returned here)
        lend = owner is not None and all(p.grad is not None for p in owner.parameters())
        if lend:
            if owner._g_scratch is None or owner._g_scratch.device != flat.device:
                owner._g_scratch = torch.empty_like(flat)
            g = owner._g_scratch.zero_()
        else:
            g = torch.zeros_like(flat)
        dhv = dhv.contiguous() if dhv is not None else torch.zeros((ctx.T * ctx.N, h.A + 1), device=flat.device)
        dhf = dh_final.contiguous() if dh_final is not None else None
        h.backward(flat, feat, masks, ctx.T, ctx.N, ws, dhv, dhf, g, feat2=ctx.feat2)
        grads = tuple(g[o:o + k].view(h.shapes[n]) for n, (o, k) in h.offsets.items())
        return (None,) * 11 + grads


class _Holder(nn.Module):
    """Creates parameter sub-module paths like ``goal_visual_encoder.resnet_compressor.0.weight``."""


def _set_nested(root: nn.Module, dotted: str, p: nn.Parameter):
    parts = dotted.split(".")
    m = root
    for part in parts[:-1]:
        if not hasattr(m, part):
            m.add_module(part, _Holder())
        m = getattr(m, part)
    m.register_parameter(parts[-1], p)


class _FlatBucketActorCritic(ActorCriticModel):
    """What every drop-in model class shares: the parameters are views of ONE flat buffer (``self._flat``) in the order of
    ``self.handle``, their ``.grad``s views of one flat gradient bucket (``self._flat_grad``), and ``_PolicyFn`` may borrow
    ``self._g_scratch``.  A subclass sets ``handle``, calls ``_adopt(state_dict, device)`` once, and ``ensure_flat()`` at the
    top of ``forward``."""

    def _adopt(self, state_dict: Dict[str, torch.Tensor], device) -> None:
        """Flatten ``state_dict`` on ``device`` and register every tensor of the handle's table as a Parameter view."""
        self._g_scratch: Optional[torch.Tensor] = None
        self._flat = self.handle.flatten(state_dict, torch.device(device))
        self._flat_grad = torch.zeros_like(self._flat)
        for name, v in self.handle.views(self._flat).items():
            _set_nested(self, name, nn.Parameter(v))
        self._bind_grads()

    # -- flat bucket maintenance -----------------------------------------------------------------
    def _named(self):
        """[(name, Parameter)] in the handle's order.  Cached: ``named_parameters()`` walks the module tree (~0.2 ms of host
        time per call, three calls per forward -- it showed in the act step of the plugin route); the Parameter OBJECTS are
        stable (``.to()`` / ``load_state_dict`` change ``.data`` in place), and ``_apply`` / ``register_parameter`` drop the
        cache in case a caller replaces them."""
        c = self.__dict__.get("_named_cache")
        if c is None:
            d = dict(self.named_parameters())
            c = self.__dict__["_named_cache"] = [(n, d[n]) for n in self.handle.param_order]
        return c

    def _apply(self, fn, *args, **kwargs):
        self.__dict__["_named_cache"] = None
        return super()._apply(fn, *args, **kwargs)

    def register_parameter(self, name, param):
        self.__dict__["_named_cache"] = None
        return super().register_parameter(name, param)

    def _bind_grads(self):
        """(Re)bind every ``p.grad`` to its view of the flat gradient bucket.  ``optimizer.zero_grad()`` of recent
        torch sets grads to None: the view is then zeroed and bound again; a foreign grad tensor is copied in."""
        for (n, p), (_, g) in zip(self._named(), self.handle.views(self._flat_grad).items()):
            if p.grad is None:
                g.zero_()
            elif p.grad.data_ptr() != g.data_ptr():
                g.copy_(p.grad)
            else:
                continue
            p.grad = g

    def ensure_flat(self):
        """Re-establish 'parameters are views of one flat buffer' after .to()/.cuda()/load."""
        ok = all(p.data_ptr() == self._flat.data_ptr() + 4 * off and p.device == self._flat.device
                 for (n, p), (off, _) in zip(self._named(), self.handle.offsets.values()))
        if ok:
            self._bind_grads()
            return
        dev = self._named()[0][1].device
        self._flat = self.handle.flatten({n: p.data for n, p in self._named()}, dev)
        self._flat_grad = torch.zeros_like(self._flat)
        for (n, p), v in zip(self._named(), self.handle.views(self._flat).values()):
            p.data = v
        self._bind_grads()

    @property
    def flat_params(self) -> torch.Tensor:
        self.ensure_flat()
        return self._flat

    @property
    def flat_grads(self) -> torch.Tensor:
        self.ensure_flat()
        return self._flat_grad


class _ResnetTensorGoalActorCritic(_FlatBucketActorCritic):
    """What the ObjectNav and the PointNav model share: everything but the goal's type.  ``_coordinate_goal`` False: the goal
    observation is an integer id per frame (``embed_class``); True: a float vector per frame (``embed_goal``), its width
    read off the goal sensor's observation space."""
    _coordinate_goal = False

    def __init__(self, action_space, observation_space, goal_sensor_uuid: str,
                 rgb_resnet_preprocessor_uuid: Optional[str] = None, depth_resnet_preprocessor_uuid: Optional[str] = None,
                 hidden_size: int = 512, goal_dims: int = 32, resnet_compressor_hidden_out_dims=(128, 32),
                 combiner_hidden_out_dims=(128, 32), state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 device="cuda", add_prev_actions: bool = False, action_embed_size: int = 6,
                 add_prev_action_null_token: bool = False, rnn_type: str = "GRU", num_rnn_layers: int = 1):
        super().__init__(action_space=action_space, observation_space=observation_space)
        # [U] RNNStateEncoder(input, hidden, num_layers=num_rnn_layers, rnn_type=rnn_type)
        if num_rnn_layers != 1:
            raise NotImplementedError("more than one recurrent layer is not built")
        if rnn_type not in ("GRU", "LSTM"):
            raise ValueError(f"rnn_type must be 'GRU' or 'LSTM', got {rnn_type!r}")
        if rnn_type == "LSTM" and depth_resnet_preprocessor_uuid is not None:
            raise NotImplementedError("an LSTM core with a depth tower is not built (the two-tower agent keeps the GRU)")
        self.rnn_type = rnn_type
        if rgb_resnet_preprocessor_uuid is None and depth_resnet_preprocessor_uuid is None:
            raise ValueError("one of rgb_resnet_preprocessor_uuid / depth_resnet_preprocessor_uuid is required")
        self.goal_uuid = goal_sensor_uuid
        self.dual = rgb_resnet_preprocessor_uuid is not None and depth_resnet_preprocessor_uuid is not None
        self.resnet_uuid = (rgb_resnet_preprocessor_uuid if rgb_resnet_preprocessor_uuid is not None
                            else depth_resnet_preprocessor_uuid)
        self.depth_uuid = depth_resnet_preprocessor_uuid if self.dual else None
        self._hidden_size = hidden_size
        self._g_scratch: Optional[torch.Tensor] = None
        if self.resnet_uuid not in observation_space.spaces:
            raise NotImplementedError("blind agent (no visual tensor in the observation space) is not built")
        if self.dual and self.depth_uuid not in observation_space.spaces:
            raise ValueError(f"{self.depth_uuid!r} is not in the observation space")
        rs = observation_space.spaces[self.resnet_uuid].shape        # (C, S, S)
        if self.dual and tuple(observation_space.spaces[self.depth_uuid].shape) != tuple(rs):
            raise ValueError("the RGB and depth feature tensors must have the same shape")
        if self._coordinate_goal:
            if self.dual:
                raise NotImplementedError("the RGB-D PointNav encoder is not built")
            goal_kw = dict(goal_in=int(observation_space.spaces[self.goal_uuid].shape[-1]))
        else:
            goal_kw = dict(num_goals=getattr(observation_space.spaces[self.goal_uuid], "n", 12))
        # [U] VisualNavActorCritic(add_prev_actions, action_embed_size, add_prev_action_null_token): prev_action_embedder.fc.weight
        # [action_space.n (+ 1), action_embed_size], concatenated to the GRU input (restated from the published source, parity unpinned)
        self.add_prev_actions = bool(add_prev_actions)
        if self.add_prev_actions:
            if self.dual:
                raise NotImplementedError("previous actions with the RGB-D encoder are not built")
            goal_kw.update(prev_action_dims=int(action_embed_size), prev_action_null=int(bool(add_prev_action_null_token)))
        self.handle = PolicyHandle(in_channels=rs[0], spatial=rs[1], hidden=hidden_size, goal_dims=goal_dims,
                                   num_actions=action_space.n,
                                   compress_hid=resnet_compressor_hidden_out_dims[0],
                                   compress_out=resnet_compressor_hidden_out_dims[1],
                                   comb_hid=combiner_hidden_out_dims[0], comb_out=combiner_hidden_out_dims[1],
                                   dual=int(self.dual), rnn_type=rnn_type, **goal_kw)
        dev = torch.device(device)
        if state_dict is None:
            from .synthetic import policy_state_dict
            state_dict = policy_state_dict(0, **self.handle.cfg, rnn_type=rnn_type)
        self._adopt(state_dict, dev)

    # -- learn-pass feature rows ------------------------------------------------------------------
    def _bf16_rows(self, feat: torch.Tensor, T: int, N: int, slot: int = 0):
        """Learn pass over the reference's fp32 NCHW rollout storage: ``ClipResNetPreprocessor.process`` returns the
        trunk's bf16 features widened to fp32, so the storage holds values that ARE bf16 -- for such a tensor the rows
        go to the kernels as bf16 NHWC (half the bytes, the 8-wave compressor kernel and the transpose-read weight-gradient
        kernel instead of the generic fp32-operand GEMMs; the products are the same numbers).  ``ec_nchw_f32_to_nhwc_bf16``
        checks exactness while it converts; anything else keeps the fp32 path (returns None).  The converted rows are kept
        while the SAME storage (base tensor, view geometry, version counter) comes back: the update epochs of a rollout."""
        import weakref
        if (feat.dtype != torch.float32 or not feat.is_cuda or not feat.is_contiguous() or feat.requires_grad
                or feat.dim() != 5 or self.handle.cfg["in_channels"] % 64 != 0):
            return None
        c = self.handle.cfg
        if c["spatial"] ** 2 * 65 * 4 > 64 * 1024:       # the conversion kernel's LDS tile (EC_ERR_SHAPE beyond): fp32 path
            return None
        base = feat._base if feat._base is not None else feat
        try:                                             # (inference-mode tensors have no version counter)
            version = base._version
        except RuntimeError:
            return None
        # NOTE the cache key relies on the storage's VERSION COUNTER: the storage must be filled through torch ops (or through
        # RN50Trunk.to_nchw_f32(out=...), which bumps the counter itself) -- a raw-pointer write from foreign code would
        # leave stale rows here
        key = (feat.data_ptr(), tuple(feat.shape), tuple(feat.stride()), version)
        cache = getattr(self, "_rows_cache", None)
        if cache is None:
            cache = self._rows_cache = {}
        hit = cache.get(slot)
        if hit is not None and hit[0]() is base and hit[1] == key:
            return hit[2]
        rows = torch.empty((T * N, c["spatial"] ** 2, c["in_channels"]), dtype=torch.bfloat16, device=feat.device)
        flag = torch.zeros(1, dtype=torch.int32, device=feat.device)
        with _lib.tensor_guard(feat):
            rc = self.handle.lib.ec_nchw_f32_to_nhwc_bf16(feat.data_ptr(), rows.data_ptr(), T * N, c["spatial"] ** 2,
                                                          c["in_channels"], flag.data_ptr(), _lib.stream_ptr())
        if rc != 0:                                            # a geometry the fast path does not take: the fp32 path serves it
            cache[slot] = (weakref.ref(base), key, None)
            return None
        out = rows if int(flag.item()) == 0 else None          # (one host sync per rollout storage version)
        cache[slot] = (weakref.ref(base), key, out)
        return out

    # -- ActorCriticModel surface ----------------------------------------------------------------
    @property
    def recurrent_hidden_state_size(self) -> int:
        return self._hidden_size

    @property
    def num_recurrent_layers(self) -> int:
        """[U] RNNStateEncoder.num_recurrent_layers: ``num_layers * (2 if "LSTM" in rnn_type else 1)``."""
        return 2 if self.rnn_type == "LSTM" else 1

    @staticmethod
    def memory_to_state(mem: torch.Tensor) -> torch.Tensor:
        """Upstream's memory tensor ``[L, N, H]`` (L = 2 on an LSTM: h then c) -> the handle's state rows ``[N, L * H]``."""
        return memory_to_state(mem, "GRU", mem.shape[0])      # (one layer: an LSTM's [h; c] is laid out as two GRU layers' rows)

    @staticmethod
    def state_to_memory(state: torch.Tensor, L: int) -> torch.Tensor:
        """The handle's state rows ``[N, L * H]`` -> upstream's memory tensor ``[L, N, H]``."""
        return state_to_memory(state, "GRU", L)

    @property
    def is_blind(self) -> bool:
        """True if the model has no visual input ([U] ``goal_visual_encoder.is_blind``); never, once constructed."""
        return False

    def _recurrent_memory_specification(self):
        return dict(rnn=((("layer", self.num_recurrent_layers), ("sampler", None),
                          ("hidden", self.recurrent_hidden_state_size)), torch.float32))

    def forward(self, observations: Dict[str, torch.Tensor], memory: Memory, prev_actions: torch.Tensor,
                masks: torch.Tensor):
        """observations[resnet_uuid]: [T,N,C,S,S] fp32 (or bf16/fp32 channels-last [T,N,S,S,C] from
        ``ClipResNetPreprocessor.process_bf16_nhwc``); observations[goal_uuid]: [T,N] int (PointNav: [T,N,goal_in] float);
        memory 'rnn': [1,N,H] ([2,N,H] on an LSTM: h then c, converted to the handle's [N,2H] rows here only); masks: [T,N,1]; prev_actions: [T,N] or [T,N,1] integer, read only with ``add_prev_actions``.
        -> (ActorCriticOutput, Memory)."""
        self.ensure_flat()
        goal = observations[self.goal_uuid]
        T, N = masks.shape[:2]
        c = self.handle.cfg

        def to_rows(feat, slot=0):
            if feat.shape[-1] == c["in_channels"] and feat.shape[-2] == c["spatial"]:
                rows = feat.reshape(T * N, c["spatial"] ** 2, c["in_channels"]).contiguous()
            else:   # the reference's NCHW layout -> NHWC rows (lossless re-layout)
                fast = self._bf16_rows(feat, T, N, slot) if (T > 1 and torch.is_grad_enabled()) else None
                if fast is not None:
                    return fast
                rows = feat.reshape(T * N, c["in_channels"], -1).transpose(1, 2).contiguous()
            return rows if rows.dtype in (torch.bfloat16, torch.float32) else rows.float()

        rows = to_rows(observations[self.resnet_uuid])
        rows2 = None
        if self.dual:
            rows2 = to_rows(observations[self.depth_uuid], 1)
            if rows2.dtype != rows.dtype:
                rows, rows2 = rows.float(), rows2.float()
        if self._coordinate_goal:
            goal = goal.reshape(T * N, self.handle.goal_in).to(torch.float32).contiguous()
        else:
            goal = goal.reshape(T * N).to(torch.int64).contiguous()
        L = self.num_recurrent_layers
        h0 = self.memory_to_state(memory.tensor("rnn").reshape(L, N, self._hidden_size).to(torch.float32))
        m = masks.reshape(T * N).to(torch.float32).contiguous()
        prev = None
        if self.add_prev_actions:
            assert prev_actions is not None and prev_actions.numel() == T * N, "add_prev_actions=True needs prev_actions [T, N] or [T, N, 1]"
            prev = prev_actions.reshape(T * N).to(torch.int64).contiguous()
        if torch.is_grad_enabled():
            params = [p for _, p in self._named()]
            hv, h_final = _PolicyFn.apply(self.handle, self, self._flat, rows, rows2, goal, prev, h0, m, T, N, *params)
        else:   # act steps (the engine's no_grad rollout): straight to the inference plan, no autograd node, no 17-tensor argument list
            ws = torch.empty(self.handle.workspace_bytes(T, N, False), dtype=torch.uint8, device=self._flat.device)
            hv, h_final = self.handle.forward(self._flat, rows, goal, h0, m, T, N, ws, for_backward=False, feat2=rows2,
                                              prev_actions=prev)
        A = self.handle.A
        hv = hv.view(T, N, A + 1)
        out = ActorCriticOutput(distributions=CategoricalDistr(logits=hv[..., :A]), values=hv[..., A:], extras={})
        return out, memory.set_tensor("rnn", self.state_to_memory(h_final, L))


class ResnetTensorObjectNavActorCritic(_ResnetTensorGoalActorCritic):
    """[U] ``ResnetTensorObjectNavActorCritic(action_space, observation_space, goal_sensor_uuid,
    rgb_resnet_preprocessor_uuid=None, depth_resnet_preprocessor_uuid=None, hidden_size=512, goal_dims=32,
    resnet_compressor_hidden_out_dims=(128, 32), combiner_hidden_out_dims=(128, 32))`` -- an
    ``allenact...policy.ActorCriticModel`` (the real ABC when allenact is importable).

    Exactly one of the two preprocessor uuids selects the single-tower ``ResnetTensorGoalEncoder`` (RGB for the CLIP
    configs of the reference; a depth-only tower is the same arithmetic on the depth features).  Both at once is
    upstream's ``ResnetDualTensorGoalEncoder`` (RGB-D: readme_files/baselines_habitat.md:75 "replace rgb with rgbd"):
    each stream has its own compressor and combiner (parameter names ``goal_visual_encoder.{rgb,depth}_resnet_compressor.*``
    / ``{rgb,depth}_target_obs_combiner.*``), the goal embedding is shared, and ``cat([rgb_x, depth_x], dim=1)`` is
    flattened into the GRU (``ec_policy_cfg.dual``).
    """


class ResnetTensorPointNavActorCritic(_ResnetTensorGoalActorCritic):
    """[U] allenact ~v0.5.0 ``projects/pointnav_baselines/models/point_nav_models.py``
    ``ResnetTensorPointNavActorCritic(action_space, observation_space, goal_sensor_uuid, rgb_resnet_preprocessor_uuid=None,
    depth_resnet_preprocessor_uuid=None, hidden_size=512, goal_dims=32, resnet_compressor_hidden_out_dims=(128, 32),
    combiner_hidden_out_dims=(128, 32))`` -- the Habitat PointNav model the reference's readme names
    (readme_files/baselines_habitat.md:64,85-86).  Restated from the published source, parity unpinned.

    The ObjectNav model with one change: the goal is the GPS + compass sensor's float vector (polar ``(rho, phi)``, uuid
    ``target_coordinates_ind``; ``observations[goal_uuid]``: ``[T, N, goal_in]``) through ``embed_goal = nn.Linear(goal_in,
    goal_dims)`` instead of an id through ``embed_class``.  ``goal_in`` is the last dimension of the goal sensor's
    observation space (2 upstream; 3 for Habitat's ``(rho, cos -phi, sin -phi)``).  18 parameters,
    ``goal_visual_encoder.embed_goal.{weight,bias}`` first; single-tower only.
    """
    _coordinate_goal = True


class ResNetRearrangeActorCriticRNN(_FlatBucketActorCritic):
    """[U] ai2thor-rearrangement ``rearrange/baseline_models.py`` ``ResNetRearrangeActorCriticRNN(action_space, observation_space,
    rgb_uuid, unshuffled_rgb_uuid, hidden_size=512, num_rnn_layers=1, rnn_type="GRU")`` -- the model of the 1-Phase Embodied CLIP
    ResNet50 IL experiment (readme_files/baselines_ithor_rearrangement.md) and of its ImageNet twin, over ``PolicyHandle.two_view``.
    Restated from the published source, which is not under the reference tree: parity unpinned.

    Behind upstream's keywords: ``prev_action_embedding_dim`` (0: ``prev_actions`` is not read; upstream's embedder is
    ``hidden_size`` wide) with ``add_prev_action_null_token``; ``attn_hidden`` (upstream's 32); ``state_dict`` / ``device``;
    ``feature_rounding``.  ``in_channels`` and ``spatial`` are read off ``observation_space.spaces[rgb_uuid].shape``.

    Parameters carry upstream's names (``two_view_param_shapes``): ``state_dict()`` / ``load_state_dict()`` exchange checkpoints
    with upstream's model and with the ``model_state_dict`` of ``Worker(net="two_view").save_checkpoint``.

    Features.  ``observations[rgb_uuid]`` and ``observations[unshuffled_rgb_uuid]``: fp32 ``[T, N, C, s, s]`` (AllenAct's
    contract), or channels-last ``[T, N, s, s, C]`` bf16 (passed through untouched) or fp32 (cast), as ``process_bf16_nhwc``
    returns them.  The handle reads bf16 rows: fp32 NCHW tensors of both views go through ``ec_nchw_f32_pair_to_nhwc_bf16`` in
    ONE launch, which rounds to nearest even.  In the learn pass (``T > 1``, grad enabled) both views' rows are kept per storage
    version, so the epochs of one rollout convert once; act steps convert on every call.

    ``feature_rounding``: this project's preprocessors widen bf16 features to fp32, so rounding them changes nothing.  Features of
    a foreign fp32 preprocessor are not bf16 values, and the kernel raises a sticky device flag for them.
      * ``"error"`` (default): the flag is read once per learn-pass conversion and by ``check_features()``; a set flag raises
        ``ValueError``.  Act steps never read it (no host stall per env step): between two checks they RUN ON ROUNDED VALUES,
        and the next check reports it.
      * ``"nearest"``: the flag is never read; the documented deviation from upstream is round-to-nearest-even of the features.
    """

    def __init__(self, action_space, observation_space, rgb_uuid: str, unshuffled_rgb_uuid: str, hidden_size: int = 512,
                 num_rnn_layers: int = 1, rnn_type: str = "GRU", prev_action_embedding_dim: int = 0,
                 add_prev_action_null_token: bool = True, attn_hidden: int = 32,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, device="cuda", feature_rounding: str = "error"):
        super().__init__(action_space=action_space, observation_space=observation_space)
        if rnn_type not in ("GRU", "LSTM"):
            raise ValueError(f"rnn_type must be 'GRU' or 'LSTM', got {rnn_type!r}")
        if not (isinstance(num_rnn_layers, int) and 1 <= num_rnn_layers <= 4):
            raise ValueError(f"num_rnn_layers must be 1..4, got {num_rnn_layers!r}")
        if feature_rounding not in ("error", "nearest"):
            raise ValueError(f"feature_rounding must be 'error' or 'nearest', got {feature_rounding!r}")
        for uuid in (rgb_uuid, unshuffled_rgb_uuid):
            if uuid not in observation_space.spaces:
                raise ValueError(f"{uuid!r} is not in the observation space")
        rs = tuple(observation_space.spaces[rgb_uuid].shape)                     # (C, s, s)
        if tuple(observation_space.spaces[unshuffled_rgb_uuid].shape) != rs:
            raise ValueError(f"{rgb_uuid!r} and {unshuffled_rgb_uuid!r} must have the same shape, got {rs} and "
                             f"{tuple(observation_space.spaces[unshuffled_rgb_uuid].shape)}")
        if len(rs) != 3 or rs[1] != rs[2]:
            raise ValueError(f"the feature maps are (C, s, s), got {rs}")
        self.rgb_uuid, self.unshuffled_rgb_uuid = rgb_uuid, unshuffled_rgb_uuid
        self.rnn_type, self.num_rnn_layers = rnn_type, num_rnn_layers
        self.feature_rounding = feature_rounding
        self._hidden_size = hidden_size
        self.prev_action_embedding_dim = int(prev_action_embedding_dim)
        self.handle = PolicyHandle.two_view(in_channels=int(rs[0]), hidden=hidden_size, num_actions=action_space.n,
                                            attn_hidden=attn_hidden, prev_action_dims=self.prev_action_embedding_dim,
                                            prev_action_null=int(bool(add_prev_action_null_token)), rnn_type=rnn_type,
                                            rnn_layers=num_rnn_layers, spatial=int(rs[1]))
        if state_dict is None:
            from .synthetic import policy_state_dict
            state_dict = policy_state_dict(0, two_view=self.handle.two_view_cfg)
        self._changed: Optional[torch.Tensor] = None       # the conversion kernel's sticky flag (device int32), made on first use
        self._rows_cache: Optional[tuple] = None           # (weakref(base u), weakref(base w), key, rows u, rows w)
        self._adopt(state_dict, device)

    # -- feature rows --------------------------------------------------------------------------------
    def _flag(self, device) -> torch.Tensor:
        if self._changed is None or self._changed.device != device:
            self._changed = torch.zeros(4, dtype=torch.int32, device=device)       # (16 bytes: word 0 is the flag)
        return self._changed

    def check_features(self) -> None:
        """``feature_rounding="error"``: read the conversion kernel's flag (one host sync), clear it, and raise ``ValueError`` if a
        feature since the last check was not a bf16 value.  Call it wherever a stall is affordable, e.g. once per rollout."""
        if self.feature_rounding != "error" or self._changed is None:
            return
        if int(self._changed[0].item()) != 0:
            self._changed.zero_()
            raise ValueError(
                f"observations {self.rgb_uuid!r} / {self.unshuffled_rgb_uuid!r} hold fp32 values that are not bf16 values: the "
                "two-view kernels read bf16 features and have been given the values rounded to nearest even.  Use this project's "
                "ClipResNetPreprocessor / ResNetPreprocessor (their fp32 output is widened bf16), or construct the model with "
                "feature_rounding='nearest' to accept the rounding.")

    def _pair_rows(self, u: torch.Tensor, w: torch.Tensor, rows: int):
        """fp32 NCHW ``[T, N, C, s, s]`` x 2 -> bf16 rows ``[rows, S2, C]`` x 2 in one launch; never reads the flag."""
        c = self.handle.cfg
        S2, Cin = c["spatial"] ** 2, c["in_channels"]
        u, w = u.contiguous(), w.contiguous()
        out = torch.empty((2, rows, S2, Cin), dtype=torch.bfloat16, device=u.device)
        with _lib.tensor_guard(u):
            _lib.check(self.handle.lib.ec_nchw_f32_pair_to_nhwc_bf16(u.data_ptr(), w.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                                     rows, S2, Cin, self._flag(u.device).data_ptr(), _lib.stream_ptr()),
                       "ec_nchw_f32_pair_to_nhwc_bf16")
        return out[0], out[1]

    @staticmethod
    def _storage_key(t: torch.Tensor):
        base = t._base if t._base is not None else t
        try:                                             # (inference-mode tensors have no version counter)
            version = base._version
        except RuntimeError:
            return base, None
        return base, (t.data_ptr(), tuple(t.shape), tuple(t.stride()), version)

    def _rows(self, u: torch.Tensor, w: torch.Tensor, T: int, N: int):
        c = self.handle.cfg
        s, Cin = c["spatial"], c["in_channels"]
        nchw, nhwc = (T, N, Cin, s, s), (T, N, s, s, Cin)
        for uuid, t in ((self.rgb_uuid, u), (self.unshuffled_rgb_uuid, w)):
            if tuple(t.shape) not in (nchw, nhwc) or t.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"observation {uuid!r}: fp32 {list(nchw)}, or bf16 / fp32 channels-last {list(nhwc)}; got "
                                 f"{t.dtype} {list(t.shape)}")
        # (C == s makes the two shapes one: an fp32 tensor is then AllenAct's NCHW, a bf16 one the preprocessor's channels-last)
        last = [tuple(t.shape) == nhwc and not (nchw == nhwc and t.dtype == torch.float32) for t in (u, w)]
        if all(last):        # channels-last: bf16 as it is, fp32 cast
            return tuple(t.reshape(T * N, s * s, Cin).to(torch.bfloat16).contiguous() for t in (u, w))
        if any(last) or u.dtype != torch.float32 or w.dtype != torch.float32 or u.device != w.device:
            raise ValueError(f"observations {self.rgb_uuid!r} and {self.unshuffled_rgb_uuid!r} must come in the same form on one "
                             f"device, fp32 {list(nchw)} or channels-last {list(nhwc)} (bf16 only channels-last)")
        if not (T > 1 and torch.is_grad_enabled()):
            return self._pair_rows(u, w, T * N)          # act step: every call, no flag read
        # learn pass: the rows of both views are kept while the SAME storages (base tensor, view geometry, version counter) come
        # back -- the update epochs of one rollout.  As on _bf16_rows, the key relies on the version counter: the storage must be
        # filled through torch ops (or RN50Trunk.to_nchw_f32(out=...), which bumps the counter itself)
        import weakref
        (bu, ku), (bw, kw) = self._storage_key(u), self._storage_key(w)
        hit = self._rows_cache
        if (hit is not None and ku is not None and kw is not None and hit[0]() is bu and hit[1]() is bw and hit[2] == (ku, kw)):
            return hit[3], hit[4]
        self._rows_cache = None
        ru, rw = self._pair_rows(u, w, T * N)
        self.check_features()                            # (one host sync per rollout storage version; "nearest": none)
        if ku is not None and kw is not None:
            self._rows_cache = (weakref.ref(bu), weakref.ref(bw), (ku, kw), ru, rw)
        return ru, rw

    # -- ActorCriticModel surface ----------------------------------------------------------------
    @property
    def recurrent_hidden_state_size(self) -> int:
        return self._hidden_size

    @property
    def num_recurrent_layers(self) -> int:
        """[U] RNNStateEncoder.num_recurrent_layers: ``num_layers * (2 if "LSTM" in rnn_type else 1)``."""
        return self.num_rnn_layers * (2 if self.rnn_type == "LSTM" else 1)

    def _recurrent_memory_specification(self):
        return dict(rnn=((("layer", self.num_recurrent_layers), ("sampler", None),
                          ("hidden", self.recurrent_hidden_state_size)), torch.float32))

    def forward(self, observations: Dict[str, torch.Tensor], memory: Memory, prev_actions: torch.Tensor,
                masks: torch.Tensor):
        """observations[rgb_uuid], observations[unshuffled_rgb_uuid]: see the class docstring; memory 'rnn': ``[L, N, H]`` (GRU) or
        ``[2L, N, H]`` (LSTM: every layer's h, then every layer's c); masks: ``[T, N, 1]``; prev_actions: ``[T, N]`` or
        ``[T, N, 1]`` integer, read only with ``prev_action_embedding_dim > 0``.  -> (ActorCriticOutput, Memory)."""
        self.ensure_flat()
        T, N = masks.shape[:2]
        h = self.handle
        rows_u, rows_w = self._rows(observations[self.rgb_uuid], observations[self.unshuffled_rgb_uuid], T, N)
        k = self.num_recurrent_layers
        h0 = h.memory_to_state(memory.tensor("rnn").reshape(k, N, self._hidden_size).to(torch.float32))
        m = masks.reshape(T * N).to(torch.float32).contiguous()
        prev = None
        if self.prev_action_embedding_dim:
            assert prev_actions is not None and prev_actions.numel() == T * N, \
                "prev_action_embedding_dim > 0 needs prev_actions [T, N] or [T, N, 1]"
            prev = prev_actions.reshape(T * N).to(torch.int64).contiguous()
        if torch.is_grad_enabled():
            params = [p for _, p in self._named()]
            hv, h_final = _PolicyFn.apply(h, self, self._flat, rows_u, rows_w, None, prev, h0, m, T, N, *params)
        else:   # act steps: straight to the inference plan, no autograd node
            ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=self._flat.device)
            hv, h_final = h.forward(self._flat, rows_u, None, h0, m, T, N, ws, for_backward=False, feat2=rows_w, prev_actions=prev)
        A = h.A
        hv = hv.view(T, N, A + 1)
        out = ActorCriticOutput(distributions=CategoricalDistr(logits=hv[..., :A]), values=hv[..., A:], extras={})
        return out, memory.set_tensor("rnn", h.state_to_memory(h_final))
