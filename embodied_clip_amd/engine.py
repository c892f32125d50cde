"""One DD-PPO worker on one MI355X: rollout storage + the two hot loops.

This is the per-GPU body of [U] AllenAct ``OnPolicyTrainer.run_pipeline``
(launched by the reference at
readme_files/baselines_robothor_objectnav.md:48-51) reduced to its
data-parallel hot path:

  HOT LOOP A (act), x T:  frames -> frozen CLIP encoder -> policy act step -> sample
  GAE returns + advantage normalisation
  HOT LOOP B (learn), x update_repeats: policy forward over [T,N] -> PPO loss ->
      backward -> (grad *= local/global) -> ONE flat-bucket RCCL all-reduce -> clip + Adam

Everything between the simulator's frames and the optimiser update runs in
the HIP library through the C-ABI; torch supplies device memory, the stream
and ``torch.distributed`` (backend "nccl" == RCCL over xGMI).  The simulator
itself is out of scope: ``SyntheticEnv`` plays pre-rendered frame batches that
are already resident in HBM.

Rollout storage layout (the encoder writes straight into it):
  feat    bf16 [T+1, N, S*S, C]   channels-last rows == the compressor GEMM's A operand
  memory  f32  [N, H] at rollout start; masks f32 [T+1, N]; goal i64 [T+1, N]
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional

import os
import random

import torch

from . import _lib
from . import synthetic as syn
from .dist import (allreduce_flat, check_job_seed, collective_active, gather_actor_counts, global_minibatch_sizes,
                   minibatch_bounds)
from .episodes import EpisodeTracker, NavEpisodeTracker, nav_env_tensors
from .encoder import AttentionPool, ClipTextEncoder, ImageNetBasicTrunk, ImageNetRN50Trunk, RN50Trunk, ViTEmbedder
from .policy import PolicyHandle
from .imitation import imitation_loss_raw, imitation_scratch
from .ppo import PPO_NARROW_MAX_A, FlatAdam, linear_decay_lr, ppo_loss_raw, ppo_wide_scratch

# encoder name -> (blocks per layer, torchvision block type, trunk class) of the ImageNet-feature agents
IMAGENET_ENCODERS = {
    "imagenet_rn18": ((2, 2, 2, 2), "basic", ImageNetBasicTrunk),
    "imagenet_rn34": ((3, 4, 6, 3), "basic", ImageNetBasicTrunk),
    "imagenet_rn50": ((3, 4, 6, 3), "bottleneck", ImageNetRN50Trunk),
}


def _frame_pool(base: torch.Tensor, pool_steps: int) -> torch.Tensor:
    """[P, N, R, R, c]: pool entry s is the base batch shifted by s + 1 actors and 7 (s + 1) columns, so consecutive steps differ."""
    return torch.stack([base.roll(shifts=s + 1, dims=0).roll(shifts=7 * (s + 1), dims=2) for s in range(pool_steps)])


class SyntheticEnv:
    """N synthetic actors: a pool of pre-rendered, CLIP-normalised 224x224 frames in HBM,
    random goal ids, episode resets w.p. 1/100, RoboTHOR-style rewards."""

    def __init__(self, n_actors: int, T: int, device, seed: int, pool_steps: int = 4, res: int = 224,
                 frames_u8: bool = False, host: bool = False, goal_in: int = 0, depth: bool = False, expert: bool = False,
                 num_actions: int = 6, sensors: int = 0, goal_view: bool = False):
        self.N, self.T = n_actors, T
        self.host = host
        # frames_u8: raw uint8 frames (what the simulator renders); normalisation is then fused into the stem kernel.
        # Every actor has its OWN frame in every pool entry (n_actors distinct images per env step: no replicated
        # images flattering the cache hit rates of the stem); the pool entries are shifted copies of one another, so
        # consecutive steps differ.  The fp32 wire form is the same arithmetic as synthetic.normalize_rgb.
        base = syn.synthetic_rgb_u8(seed, n_actors, res)
        if not frames_u8:   # (on the device when the pool lives there: 256 frames take 6 s on the host)
            base = syn.normalize_rgb(base if host else base.to(device))
        frames = _frame_pool(base, pool_steps)
        # host=True: the pool stays in PINNED HOST memory (what the simulators hand over through the plugin contract);
        # the worker then streams each step's frames over PCIe on a copy stream (Worker._encode_slice)
        self.frames = (frames.contiguous().pin_memory() if host else frames.to(device).contiguous())   # [P, N, R, R, 3] fp32 | uint8
        self.pool_steps = pool_steps
        masks = torch.cat([torch.ones(1, n_actors, 1), syn.synthetic_masks(seed + 1, T, n_actors)], 0)
        self.masks = masks.reshape(T + 1, n_actors).to(device).contiguous()
        # goal_in > 0 (PointNav): float [T+1, N, goal_in] coordinate goals (distance, bearing) instead of int64 ids [T+1, N]
        goals = (syn.synthetic_goal_vectors(seed + 2, (T + 1, n_actors), goal_in) if goal_in
                 else syn.synthetic_goals(seed + 2, (T + 1, n_actors)))
        self.goals = goals.to(device).contiguous()
        if expert:
            # imitation learning: the expert's action (a function of the goal) and whether it has one, [T+1, N] each, from a
            # seed and a hash stream of their own (synthetic.synthetic_expert) -- nothing else the env builds changes
            ea, em = syn.synthetic_expert(seed + 6, goals, num_actions)
            self.expert_actions, self.expert_mask = ea.to(device).contiguous(), em.to(device).contiguous()
        self.rewards = syn.synthetic_rewards(seed + 3, masks[1:]).reshape(T, n_actors).to(device).contiguous()
        # success flag of the step that ends an episode: the +10 reward of synthetic_rewards (episode metrics / evaluation)
        self.success = ((self.rewards > 1) & (self.masks[1:] == 0)).to(torch.float32).contiguous()
        # the second per-step input, served by observe_second(): the depth frames or the goal-state views (an env built with both
        # serves the goal views there; observe_depth() / observe_goal_view() name either)
        self._second = None
        if depth:
            # RGB-D: one-channel depth frames from a hash stream of their own, normalised (synthetic.normalize_depth), with
            # the frames' construction
            dbase = syn.normalize_depth(syn.synthetic_depth(seed + 5, n_actors, res).to(device))
            self.depth = self._second = _frame_pool(dbase, pool_steps).contiguous()   # [P, N, R, R, 1] fp32
        if sensors:
            # the pooled-embedding net's small float sensors (GPS, compass, a 3-float point goal): K floats per actor and step,
            # f32 [T+1, N, K], from a seed of their own -- nothing else the env builds changes
            self.sensors = torch.randn(T + 1, n_actors, int(sensors), generator=torch.Generator().manual_seed(seed + 8)).to(device).contiguous()
        if goal_view:
            # the two-view rearrangement net: a second RGB frame per actor and step, the view of the GOAL state from the same pose, in
            # the frames' wire form and construction, from a seed and hash stream of its own -- nothing else the env builds changes
            gbase = syn.synthetic_rgb_u8(seed + 9, n_actors, res).to(device)
            if not frames_u8:
                gbase = syn.normalize_rgb(gbase)
            self.goal_frames = self._second = _frame_pool(gbase, pool_steps).contiguous()   # [P, N, R, R, 3] fp32 | uint8, on the device
        self._k = 0

    def observe(self, actions_host: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Next batch of frames.  ``actions_host`` (the sampled actions, on the host) is what a simulator would consume;
        the synthetic env only requires that it has arrived."""
        f = self.frames[self._k % self.pool_steps]
        self._k += 1
        return f

    def observe_at(self, k: int, actions_host: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The batch ``observe()`` serves as its k-th call (per-slice env stepping: every slice asks for step k itself)."""
        return self.frames[k % self.pool_steps]

    def observe_second(self, pool: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The second input that goes with the frames ``observe()`` served last: the depth batch (``depth=True`` envs) or the
        goal-state views (``goal_view=True`` envs)."""
        return self.observe_second_at(self._k - 1, pool)

    def observe_second_at(self, k: int, pool: Optional[torch.Tensor] = None) -> torch.Tensor:
        """... that goes with ``observe_at(k)``."""
        return (self._second if pool is None else pool)[k % self.pool_steps]

    # (the pair above under the names of what it serves, for tools and tests)
    def observe_depth(self) -> torch.Tensor:
        return self.observe_second(self.depth)

    def observe_depth_at(self, k: int) -> torch.Tensor:
        return self.observe_second_at(k, self.depth)

    def observe_goal_view(self) -> torch.Tensor:
        return self.observe_second(self.goal_frames)

    def observe_goal_view_at(self, k: int) -> torch.Tensor:
        return self.observe_second_at(k, self.goal_frames)


class NavSyntheticEnv(SyntheticEnv):
    """``SyntheticEnv`` (the same frames, masks, goals, rewards, success) plus the geometry the navigation metrics read:
    ``step_dist`` / ``start_dist`` / ``goal_dist`` f32 [T, N] (``synthetic.synthetic_navigation``, hash streams of its own) and
    ``num_goals``, the number of goal ids (0 with coordinate goals)."""

    def __init__(self, n_actors: int, T: int, device, seed: int, pool_steps: int = 4, res: int = 224,
                 frames_u8: bool = False, host: bool = False, goal_in: int = 0, depth: bool = False, expert: bool = False,
                 num_actions: int = 6, sensors: int = 0, goal_view: bool = False):
        super().__init__(n_actors, T, device, seed, pool_steps, res, frames_u8, host, goal_in, depth, expert, num_actions, sensors, goal_view)
        self.num_goals = 0 if goal_in else 12
        step_dist, start_dist, goal_dist = syn.synthetic_navigation(seed + 4, self.masks[1:], self.success)
        self.step_dist = step_dist.to(device).contiguous()
        self.start_dist = start_dist.to(device).contiguous()
        self.goal_dist = goal_dist.to(device).contiguous()


class _Slice:
    """Per-slice state: a contiguous group of actors with its own stream, encoder handle and buffers."""
    pass


def check_prev_actions(prev_actions: int, depth: bool, zeroshot: bool, max_dims: int = 64) -> int:
    """``Worker`` / ``Evaluator`` ``(prev_actions=E)``: the embedding's width, refused where the policy library refuses it
    (``max_dims``: 512 on the two-view net, whose upstream width is the hidden size)."""
    E = int(prev_actions)
    if not 0 <= E <= max_dims:
        raise ValueError(f"prev_actions={prev_actions}: the embedding's width is 0 (off) or 1..{max_dims}")
    if E and depth:
        raise ValueError("prev_actions > 0 with depth=True: the dual (RGB + depth) goal encoder with previous actions is not built")
    if E and zeroshot:
        raise ValueError("prev_actions > 0 with zeroshot=True: the zero-shot fusion policy with previous actions is not built")
    return E


def check_rnn_type(rnn_type: str, depth: bool, zeroshot: bool) -> str:
    """``Worker`` / ``Evaluator`` ``(rnn_type=...)``: the recurrent cell, refused where the policy library refuses it; raised
    before anything is allocated."""
    if rnn_type not in ("GRU", "LSTM"):
        raise ValueError(f"rnn_type={rnn_type!r}: 'GRU' or 'LSTM'")
    if rnn_type == "LSTM" and depth:
        raise ValueError("rnn_type='LSTM' with depth=True: the two-tower (RGB + depth) agent keeps the GRU; an LSTM core for it is not built")
    if rnn_type == "LSTM" and zeroshot:
        raise ValueError("rnn_type='LSTM' with zeroshot=True: the zero-shot fusion policy keeps the GRU; an LSTM core for it is not built")
    return rnn_type


def check_rnn_layers(rnn_layers: int, depth: bool, zeroshot: bool) -> int:
    """``Worker`` / ``Evaluator`` ``(rnn_layers=L)``: the recurrent depth ([U] RNNStateEncoder ``num_layers``), refused where the
    policy library refuses it; raised before anything is allocated."""
    if not (isinstance(rnn_layers, int) and not isinstance(rnn_layers, bool) and 1 <= rnn_layers <= 4):
        raise ValueError(f"rnn_layers={rnn_layers!r}: an integer in 1..4")
    if rnn_layers > 1 and depth:
        raise ValueError("rnn_layers > 1 with depth=True: the two-tower (RGB + depth) agent keeps one recurrent layer")
    if rnn_layers > 1 and zeroshot:
        raise ValueError("rnn_layers > 1 with zeroshot=True: the zero-shot fusion policy keeps one recurrent layer")
    return rnn_layers


def check_rgbd(encoder: str, zeroshot: bool, goal_in: int, frames_host: bool) -> None:
    """What ``depth=True`` (the RGB-D agent) cannot be combined with; raised before anything is allocated."""
    if encoder not in ("rn50", "rn50x16"):
        raise ValueError(f"depth=True: the one-channel depth stem exists for the CLIP ResNet towers (encoder 'rn50' / 'rn50x16'), not {encoder!r}")
    if zeroshot:
        raise ValueError("depth=True: the zero-shot agent fuses ONE image embedding with the text embedding; it has no depth stream")
    if goal_in:
        raise ValueError("depth=True: the dual (RGB + depth) goal encoder takes goal ids; coordinate goals (goal_in > 0) are unsupported by the policy library")
    if frames_host:
        raise ValueError("depth=True: host-resident frames (frames_host=True) have no depth staging path")


def check_net(net: str, pooling: str, sensors, goal_ids: bool, encoder: str, depth: bool, zeroshot: bool, goal_in: int):
    """``Worker`` / ``Evaluator`` ``(net=..., pooling=..., sensors=..., goal_ids=...)``: "goal_encoder" (the default: AllenAct's
    ResnetTensorGoalEncoder agent) or "pooled" (habitat-lab's PointNavResNetNet over the pooled embedding, ``PolicyHandle.pooled``).
    "two_view": the rearrangement agent ([U] ResNetRearrangeActorCriticRNN, ``PolicyHandle.two_view``) -- a pooled plan over the
    feature MAPS of two views: no goal input at all, so it returns (True, None, ()) and its users clear ``goal_ids``.
    Raised before anything is allocated.  -> (pooled, pooling, sensors)"""
    if net not in ("goal_encoder", "pooled", "two_view"):
        raise ValueError(f"net={net!r}: 'goal_encoder', 'pooled' or 'two_view'")
    if net == "two_view":
        if depth:
            raise ValueError("net='two_view' with depth=True: the second feature buffer holds the goal view; an RGB-D rearrangement agent is not built")
        if zeroshot:
            raise ValueError("net='two_view' with zeroshot=True: the zero-shot fusion policy is another net")
        if goal_in:
            raise ValueError("net='two_view' with goal_in > 0: the goal IS the second view; the net has no coordinate goal")
        if tuple(sensors):
            raise ValueError("net='two_view' with sensors=...: float sensors belong to net='pooled'")
        if not goal_ids:
            raise ValueError("net='two_view' with goal_ids=False: the switch belongs to net='pooled' (this net has no goal-id input either way)")
        if pooling != "attnpool":
            raise ValueError("net='two_view' with pooling=...: the net reads the 7 x 7 feature maps and pools them itself")
        if encoder == "vit":
            raise ValueError("net='two_view' with encoder='vit': the ViT's patch tokens as a second view are not built")
        return True, None, ()
    if net == "goal_encoder":
        if tuple(sensors):
            raise ValueError("sensors=... belongs to net='pooled'")
        return False, None, ()
    sensors = tuple(int(k) for k in sensors)
    if pooling not in ("attnpool", "avgpool", "cls"):
        raise ValueError(f"pooling={pooling!r}: 'attnpool', 'avgpool' or 'cls'")
    if pooling == "cls" and encoder != "vit":
        raise ValueError(f"pooling='cls' is the ViT's class embedding ([U] ClipViTPreprocessor, class_emb_only): encoder='vit', not {encoder!r}")
    if depth and pooling != "avgpool":
        # [U] ResNetCLIPEncoder removes the attention pool when it encodes rgb + depth: the two maps are summed and average-pooled
        raise ValueError("net='pooled' with depth=True: the RGB-D encoder sums the two towers' maps and average-pools them; use pooling='avgpool'")
    if depth and encoder in IMAGENET_ENCODERS:
        raise ValueError(f"net='pooled' with depth=True: the 7x7 stem of {encoder!r} has no one-channel form; encoder='rn50'")
    if zeroshot:
        raise ValueError("net='pooled' with zeroshot=True: the zero-shot fusion policy is another net")
    if goal_in:
        raise ValueError("net='pooled' with goal_in > 0: coordinate goals reach the pooled net as sensors=(k,)")
    if encoder == "vit" and pooling != "cls":
        raise ValueError(f"net='pooled' with encoder='vit', pooling={pooling!r}: the ViT has no attention pool and no feature map to average; "
                         "use pooling='cls' (its class embedding)")
    if encoder in IMAGENET_ENCODERS and pooling == "attnpool":
        raise ValueError("net='pooled', pooling='attnpool': the ImageNet towers have no attention pool; use pooling='avgpool'")
    if encoder not in ("rn50", "vit") and encoder not in IMAGENET_ENCODERS:
        raise ValueError(f"net='pooled': encoder 'rn50' ('attnpool' / 'avgpool'), an ImageNet tower ('avgpool') or 'vit' ('cls'), not {encoder!r}")
    if len(sensors) > 3 or any(k < 1 for k in sensors) or sum(sensors) > 8:
        raise ValueError(f"sensors={sensors!r}: at most 3 sensors of at least one float each, 8 floats in all")
    if not goal_ids and not sensors:
        raise ValueError("net='pooled' needs a goal: goal_ids=True or at least one sensor")
    return True, pooling, sensors


def check_model_tensors(policy, sd, where: str) -> None:
    """A checkpoint's ``model_state_dict`` against the handle's tensors: a missing one (a checkpoint written without the
    previous-action embedding, loaded by an agent that has it) raises, naming the tensor and the file; so does one whose
    element count differs (a GRU checkpoint's ``3H``-row recurrent tensors into an LSTM agent, or the reverse), naming both shapes."""
    for name in sd:                     # a deeper checkpoint: an upper recurrent layer this agent does not have
        if name.startswith("state_encoder.rnn.") and name not in policy.offsets:
            raise ValueError(f"{where}: the checkpoint's tensor {name!r} {tuple(sd[name].shape)} belongs to a recurrent layer this agent "
                             f"does not have (rnn_layers={getattr(policy, 'rnn_layers', 1)})")
    for name in policy.offsets:
        if name not in sd:
            raise KeyError(f"{where}: the checkpoint lacks the tensor {name!r} {tuple(policy.shapes[name])} of this agent")
    for name in policy.offsets:         # (behind the missing-tensor check: an agent's extra tensor is named first)
        want = tuple(policy.shapes[name])
        n = 1
        for dim in want:
            n *= dim
        if sd[name].numel() != n:       # e.g. a GRU checkpoint's [3H, .] recurrent tensors into an LSTM agent's [4H, .], or the reverse
            raise ValueError(f"{where}: the tensor {name!r} is {tuple(sd[name].shape)} in the checkpoint and {want} in this agent "
                             f"(rnn_type={getattr(policy, 'rnn_type', 'GRU')!r})")


class _SlicedActor:
    """What a training ``Worker`` and an ``evaluate.Evaluator`` share: the frozen encoder handles and the policy handle, the
    actor slices with their streams, act workspaces and feature buffers, and hot loop A's encode step.  The users call
    ``_configure`` (the agent description) first, set ``self.dev`` / ``self.device``, ``self.nav_metrics``, ``self._text_sd`` and
    ``self._goal_tokens``, and set ``self.env`` between ``_build_model`` and ``_build_slices``.

    ``self.depth`` (an RGB-D agent, readme_files/baselines_habitat.md:75): the env serves depth frames and ``_observe`` hands
    them to the encode step.  What the agent does with them is ``self.dual``:

    * ``dual`` (``depth`` with the goal-encoder net; [U] AllenAct's two preprocessors): every slice's trunk handle also encodes
      the depth batch (``RN50Trunk.forward_depth``: same frozen weights, one-channel stem) into a second feature buffer
      ``sl.feat2``, and the policy is the dual-encoder variant.
    * ``depth`` with the pooled net ([U] habitat branch ``ResNetCLIPEncoder``): ``RN50Trunk.embed_rgbd`` encodes both frames of
      a pair in one pass into ONE vector; no second buffer, and the policy is the RGB pooled net's."""
    depth = False

    # net="two_view" (check_net): the rearrangement agent -- the env also serves the goal-state view, every slice encodes it with its
    # one trunk handle into ``sl.feat2`` (the RGB-D agent's second buffer), and the policy is ``PolicyHandle.two_view``
    two_view_net = False

    @property
    def dual(self) -> bool:
        return (self.depth and not self.pooled_net) or self.two_view_net
    # the previous action's embedding ([U] VisualNavActorCritic add_prev_actions / Habitat's prev_action_embedding): its width
    # (0: off) and whether row 0 is the null token of an episode's first step; set by the users before ``_build_model``
    prev_action_dims = 0
    prev_action_null = 0
    # the recurrent cell ([U] RNNStateEncoder rnn_type): "LSTM" makes every recurrent-memory buffer [N, 2H] rows [h | c]
    rnn_type = "GRU"
    # recurrent layers ([U] RNNStateEncoder num_layers): a memory row is [N, L * SW], layer-major
    rnn_layers = 1
    hidden_size = 512       # the recurrent width ([U] hidden_size); ``Worker`` / ``Evaluator`` ``(hidden=...)``
    # net="pooled" (check_net): the pooled-embedding net over one vector per frame -- how the tower is pooled, the widths of the
    # env's float sensors, whether the goal id is embedded; set by the users before ``_build_model``
    pooled_net = False
    pooling = None
    net_sensors = ()
    goal_ids = True

    # how a frame becomes ONE fp32 vector in the rollout buffer: "attnpool" (the zero-shot agent, the pooled net), "avgpool" (the
    # pooled net), or None (feature maps); ``_build_model`` sets it
    _embed = None

    def _configure(self, encoder, net, pooling, sensors, goal_ids, goal_in, depth, zeroshot, num_actions, prev_actions,
                   prev_action_null_token, rnn_type, rnn_layers, hidden, frames_host=False, env=None):
        """The agent description: every refusal, then the attributes the rest of the class reads.  Called first by both users, so a
        refused combination raises before anything is allocated or the library is loaded.  ``frames_host``: the Worker's;
        ``env``: the Evaluator's optional ``env=``, which must serve what the agent reads."""
        host = bool(frames_host or (env is not None and getattr(env, "host", False)))
        self.pooled_net, self.pooling, self.net_sensors = check_net(net, pooling, sensors, goal_ids, encoder, bool(depth), bool(zeroshot), goal_in)
        self.two_view_net = net == "two_view"
        self.goal_ids = bool(goal_ids) and not self.two_view_net
        if self.two_view_net and frames_host:
            raise ValueError("net='two_view': host-resident frames (frames_host=True) have no staging path for the goal view")
        if self.two_view_net and env is not None and (getattr(env, "goal_frames", None) is None or host):
            raise ValueError("net='two_view': the env serves no goal-state views on the device (SyntheticEnv(..., goal_view=True) holds env.goal_frames)")
        if self.net_sensors and env is not None and getattr(env, "sensors", None) is None:
            raise ValueError("net='pooled' with sensors: the env serves no sensor vectors (SyntheticEnv(..., sensors=K) holds env.sensors)")
        if depth:
            check_rgbd(encoder, zeroshot, goal_in, host)
            if env is not None and getattr(env, "depth", None) is None:
                raise ValueError("depth=True: the env serves no depth frames (SyntheticEnv(..., depth=True) holds env.depth)")
        two_tower = bool(depth) and not self.pooled_net     # (the pooled RGB-D agent's policy handle is the RGB pooled net's: nothing to refuse)
        self.prev_action_dims = check_prev_actions(prev_actions, two_tower, bool(zeroshot), 512 if self.two_view_net else 64)
        self.prev_action_null = int(bool(prev_action_null_token)) if self.prev_action_dims else 0
        self.rnn_type = check_rnn_type(rnn_type, two_tower, bool(zeroshot))
        self.rnn_layers = check_rnn_layers(rnn_layers, two_tower, bool(zeroshot))
        self.hidden_size = int(hidden)
        self.depth = bool(depth)
        assert not (goal_in and zeroshot), "coordinate goals go through the goal encoder, not the zero-shot fusion"
        self.zeroshot, self.goal_in, self._num_actions = zeroshot, goal_in, num_actions
        # what the policy calls of this agent take beside the features (read per step as plain attributes): the env's goal rows
        # (not on a pooled net without the goal-id embedding, nor on the two-view net) and the pooled net's sensor rows
        self._has_goal = self.goal_ids or not self.pooled_net
        self._has_sensors = bool(self.net_sensors)
        self._has_second = self.depth or self.two_view_net      # the env's second per-step input: depth frames / goal-state views
        self.lib = _lib.load()

    def _env_recipe(self, expert: bool = False):
        """The env this agent reads.  -> (class, keywords beside the sizes, the seed and the frames' form)"""
        kw = dict(goal_in=self.goal_in)
        if self.depth:
            kw["depth"] = True
        if expert:
            kw.update(expert=True, num_actions=self._num_actions)
        if self.net_sensors:
            kw["sensors"] = sum(self.net_sensors)
        if self.two_view_net:
            kw["goal_view"] = True
        return (NavSyntheticEnv if self.nav_metrics else SyntheticEnv), kw

    def _episode_tracker(self, num_categories=None, capacity: int = 0):
        """``nav_metrics``: per-category rows for goal ids (default: the env's ``num_goals``); coordinate goals have no categories."""
        if not self.nav_metrics:
            return EpisodeTracker(self.N, self.dev, capacity=capacity)
        C = 0 if self.goal_in else (num_categories if num_categories is not None else getattr(self.env, "num_goals", 12))
        return NavEpisodeTracker(self.N, self.dev, num_categories=C, capacity=capacity)

    def _update_episodes(self):
        """Fold the env's ``rewards`` / ``masks`` / ``success`` (and the navigation geometry) of one rollout into the tracker."""
        nav = nav_env_tensors(self.env, self.episodes.C > 0) if self.nav_metrics else ()
        self.episodes.update(self.env.rewards, self.env.masks, getattr(self.env, "success", None), *nav)

    def _encoder_handles(self, ns, make):
        """``make(weights_from)`` once, then ``ns - 1`` handles that borrow the first one's device weights."""
        share = os.environ.get("EC_SHARE_WEIGHTS", "1") != "0"
        first = make(None)
        return [first] + [make(first if share else None) for _ in range(ns - 1)]

    def _policy_recipe(self, encoder):
        """The agent's policy.  -> (constructor, its keywords, the name under which ``synthetic.policy_state_dict`` takes the same
        keywords for the seeded stand-in weights: None = as they are)"""
        rnn = dict(rnn_type=self.rnn_type, rnn_layers=self.rnn_layers)
        pa = dict(prev_action_dims=self.prev_action_dims, prev_action_null=self.prev_action_null)
        if self.two_view_net:
            return PolicyHandle.two_view, dict(in_channels=self.C, hidden=self.hidden_size, num_actions=self._num_actions, spatial=self.S,
                                               **pa, **rnn), "two_view"
        if self.pooled_net:
            return PolicyHandle.pooled, dict(embed_in=self.C, hidden=self.hidden_size, num_goals=12 if self.goal_ids else 0,
                                             sensors=self.net_sensors, num_actions=self._num_actions, **pa, **rnn), "pooled"
        kw = dict(in_channels=self.C, spatial=self.S, num_actions=self._num_actions, **rnn)
        if self.goal_in:
            kw["goal_in"] = self.goal_in
        if self.dual:      # [U] ResnetDualTensorGoalEncoder: 25 tensors, rgb_* / depth_* compressors and combiners
            kw["dual"] = 1
        if self.zeroshot:
            assert encoder == "rn50", "the zero-shot variant uses the CLIP-RN50 image embedding"
            kw["fusion"] = 1
        if self.prev_action_dims:
            kw.update(pa)
        if self.hidden_size != 512:
            kw["hidden"] = self.hidden_size
        return PolicyHandle, kw, None

    def _build_model(self, n_actors, encoder, encoder_sd, policy_sd, encoder_chunk, encoder_streams):
        """Encoder handles (one per slice, weights shared), the policy handle and its flat parameters.  -> (encs, pools)"""
        self.encoder = encoder
        self._embed = "attnpool" if self.zeroshot else self.pooling
        # two slices (each with its own act -> encode chain on its own stream) from 48 actors on: measured round 3 at
        # 32 / 48 / 64 actors, one vs two slices: 26.8 / 29.0 / 35.0 k vs 26.1 / 31.8 / 36.8 k env-frames/s
        two_min = int(os.environ.get("EC_TWO_SLICE_MIN", "48"))          # (experiment switch for the rule above)
        ns = encoder_streams if (encoder_streams > 1 and n_actors >= two_min and n_actors % encoder_streams == 0) else 1
        self.ns = ns
        d = self.dev
        pools = [None] * ns
        if encoder in ("rn50", "rn50x16"):
            # "rn50x16": CLIP RN50x16's tower (width 96, layers (6, 8, 18, 8)) on the plugin's 224 x 224 frames -> a
            # 3072 x 7 x 7 map ([U] ClipResNetPreprocessor's second model type; functional path, not tuned)
            sd = encoder_sd if encoder_sd is not None else (
                syn.rn50_visual_state_dict(0) if encoder == "rn50" else
                syn.rn50_visual_state_dict(0, width=96, layers=(6, 8, 18, 8), output_dim=768, heads=48))
            encs = self._encoder_handles(ns, lambda w: RN50Trunk(sd, device=d, chunk=encoder_chunk, weights_from=w))
            self.S, self.C = encs[0].out_spatial, encs[0].out_channels
            if self._embed == "attnpool":
                pools = self._encoder_handles(ns, lambda w: AttentionPool(sd, device=d, weights_from=w))
                self.trunk_S, self.trunk_C = self.S, self.C
                self.S, self.C = 1, pools[0].out_dim
        elif encoder in IMAGENET_ENCODERS:
            # the ImageNet baselines' torchvision trunks ([U] allenact ResNetPreprocessor: objectnav_robothor_rgb_resnet18gru_ddppo
            # / ..._resnet50gru_ddppo): ResNet-18 / 34 -> 512 x 7 x 7, ResNet-50 -> 2048 x 7 x 7, same policy and PPO
            layers, block, cls = IMAGENET_ENCODERS[encoder]
            sd = encoder_sd if encoder_sd is not None else syn.tv_resnet_state_dict(0, layers=layers, block=block)
            encs = self._encoder_handles(ns, lambda w: cls(sd, device=d, chunk=encoder_chunk, weights_from=w))
            self.S, self.C = encs[0].out_spatial, encs[0].out_channels
        elif encoder == "vit":
            # BASELINE config 3 (builder-defined fusion, SURVEY.md §8d note): ClipViTEmbedder tokens, CLS dropped,
            # the 49 patch tokens are the 7x7 channels-last "feature map" [n,49,768] of the goal encoder
            sd = encoder_sd if encoder_sd is not None else syn.vit_visual_state_dict(0)
            if self._embed == "cls":
                # the pooled net over the class embedding ([U] ClipViTPreprocessor, class_emb_only): one [D] vector per frame whatever
                # the token count, so any tower geometry of 64-wide heads (ViT-B/32, B/16, L/14) works; no token buffer
                heads = int(sd["class_embedding"].shape[0]) // 64
                encs = self._encoder_handles(ns, lambda w: ViTEmbedder(sd, device=d, heads=heads, weights_from=w))
                self.S, self.C = 1, encs[0].D
            else:
                encs = self._encoder_handles(ns, lambda w: ViTEmbedder(sd, device=d, weights_from=w))
                self.S, self.C = 7, encs[0].D
        else:
            raise ValueError(encoder)
        if self._embed == "avgpool":      # AdaptiveAvgPool2d(1) of the trunk output (ec_spatial_mean_bf16): D = the trunk's channels
            self.trunk_S, self.trunk_C = self.S, self.C
            self.S = 1
        make, pkw, sd_name = self._policy_recipe(encoder)
        self.policy = make(**pkw)
        if policy_sd is not None:   # a checkpoint of another net, cell or depth: refused by the tensor's name (and both shapes), with the file
            check_model_tensors(self.policy, policy_sd, getattr(self, "_checkpoint", None) or "policy_sd")
        if self.zeroshot:
            # goal table: the CLIP text tower over the 12 goal prompts, once, L2-normalised; frozen
            tsd = self._text_sd if self._text_sd is not None else syn.text_state_dict(0)
            tok = self._goal_tokens if self._goal_tokens is not None else syn.synthetic_tokens(
                7, 12, context_length=tsd["positional_embedding"].shape[0], vocab_size=tsd["token_embedding.weight"].shape[0])
            self.goal_table = ClipTextEncoder(tsd, device=d).goal_table(tok).contiguous()
            self.policy.set_goal_table(self.goal_table)
        self.H, self.A = self.policy.H, self.policy.A
        self.SW = self.policy.state_width        # width of a recurrent-memory row: L * H, or L * 2H ([h | c] per layer) with an LSTM core
        if policy_sd is None:       # the seeded stand-in weights
            policy_sd = syn.policy_state_dict(0, **({sd_name: pkw} if sd_name else pkw))
        self.params = self.policy.flatten(policy_sd, d)
        return encs, pools

    def _build_slices(self, n_actors, encs, pools, feat_steps, n_comm, frames_host):
        """Streams and the per-slice state hot loop A needs; ``feat_steps`` entries of feature storage per slice (T + 1: a
        training rollout; 2: the ring of an evaluation run)."""
        ns, d, encoder = self.ns, self.dev, self.encoder
        n = n_actors // ns
        S2 = self.S * self.S
        self.slices: List[_Slice] = []
        # Streams.  The HIP runtime has FOUR hardware queues and binds a stream to one of them at its first submission; two
        # streams on one queue run one after the other (a slice pair that shared a queue serialised the two encoder launches:
        # 48 instead of 63 k; a copy stream on the other slice's compute queue: 59 -> 42 k; tools/sync_probe.py, h2d_probe.py).
        # So the slices' streams, the communication stream of the overlapped all-reduce (only where there is a collective) and
        # the slices' copy streams (frames in host memory) come from ONE pool that _lib.concurrent_streams has verified pairwise
        # concurrent; when that is more than the queues allow, the copy streams, then the communication stream, go unverified.
        n_own = ns if ns > 1 else 0
        n_copy = ns if frames_host else 0
        plain = lambda k: [torch.cuda.Stream(device=d) for _ in range(k)]   # noqa: E731
        pool = None
        for take_comm, take_copy in ((n_comm, n_copy), (n_comm, 0), (0, 0)):
            want = n_own + take_comm + take_copy
            try:
                pool = (_lib.concurrent_streams(want, d) if want > 1 else plain(want))
            except RuntimeError:
                if take_comm == 0 and take_copy == 0:
                    raise
                continue
            if (take_comm, take_copy) != (n_comm, n_copy):
                import warnings
                warnings.warn(f"{n_own + n_comm + n_copy} streams exceed the runtime's hardware queues: only {want} are verified concurrent")
            pool = pool + plain(n_comm - take_comm + n_copy - take_copy)
            order = ["own"] * n_own + ["comm"] * take_comm + ["copy"] * take_copy + ["comm"] * (n_comm - take_comm) + ["copy"] * (n_copy - take_copy)
            break
        by = lambda kind: [s_ for s_, k_ in zip(pool, order) if k_ == kind]   # noqa: E731
        slice_streams = by("own") if n_own else [None]
        copy_streams = by("copy")
        self.comm_stream = by("comm")[0] if n_comm else None      # (a Worker without a collective makes itself a plain one)
        for i in range(ns):
            sl = _Slice()
            sl.o, sl.n, sl.enc, sl.pool = i * n, n, encs[i], pools[i]
            sl.stream = slice_streams[i]
            # zero-shot: the rollout buffer holds fp32 image embeddings [T+1, n, 1, 1024]; else bf16 feature maps
            sl.feat = torch.empty((feat_steps, n, S2, self.C), dtype=torch.float32 if self._embed else torch.bfloat16, device=d)
            sl.feat2 = torch.empty_like(sl.feat) if self.dual else None      # the depth tower's features
            sl.trunk_out = (torch.empty((n, self.trunk_S, self.trunk_S, self.trunk_C), dtype=torch.bfloat16, device=d)
                            if self._embed and self._embed != "cls" and not self.depth else None)   # (embed_rgbd / embed_cls keep theirs in their own workspace)
            sl.tok = (torch.empty((n, encs[i].L, encs[i].D), dtype=torch.bfloat16, device=d) if encoder == "vit" and self._embed != "cls" else None)
            sl.ws_act = torch.empty(self.policy.workspace_bytes(1, n, False), dtype=torch.uint8, device=d)
            sl.act_tables_valid = False     # weight-derived tables in ws_act (rebuilt by the first act step after an update)
            if frames_host:   # double-buffered device staging of the slice's frames + its own copy stream (SDMA)
                fshape = (n,) + tuple(self.env.frames.shape[2:])
                sl.stage = [torch.empty(fshape, dtype=self.env.frames.dtype, device=d) for _ in range(2)]
                sl.copy_stream = copy_streams[i]
                sl.copied = [torch.cuda.Event() for _ in range(2)]
                sl.consumed = [None, None]
                sl.k = 0
            self.slices.append(sl)
        self.encode_frames = n                    # frames per timed encoder launch
        # two launches in flight with >= 128 frames each: the 8-wave conv kernel from 50 tiles on -- a property of THIS
        # worker's encoder handles (ec_rn50/vit_set_conv8_min_tiles), not of the process.  With 64..127 frames per slice:
        # from 75 tiles on (round 3, after the long-segment 128-wide tiles: 128 actors 46.6-47.2 k with the default 150,
        # 48.2 k with 50, 49.2-49.3 k with 60 / 75 / 90; two slices of 32 frames keep the default: 39.1 vs 37.6 k)
        self._conv8_min_tiles = (50 if n >= 128 else (75 if n >= 64 else 0)) if ns == 2 else 0
        for e in encs:
            e.set_conv8_min_tiles(self._conv8_min_tiles)
        # CLIP RN50: layer 1's block-0 output is rebuilt at the next boundary, not stored (ec_rn50_set_l1_rebuild): bit-identical
        # features, 768 B per 56 x 56 pixel less HBM traffic.  A tower without that plan (other layer counts) says so and keeps its own
        if encoder == "rn50":
            for e in encs:
                e.set_l1_rebuild(True)
        # A/B switch.  Up to 7 actions: the narrow heads launch samples (ec_policy_act).  8 to 256: the wide heads launch computes
        # the logits, selects and forces (ec_policy_act_ex).  Off, above 256, or a hidden size whose rows do not fit the wide
        # launch's LDS (ec_heads_wide: H <= 3576): the forward, then the stand-alone selection calls
        fused = os.environ.get("EC_ACT_FUSED_SAMPLE", "1") != "0"
        self._act_fused = fused and self.A + 1 <= 8
        self._act_wide = fused and 8 < self.A + 1 <= 257 and self.H <= 3576
        self.trunk_events: List = []             # (start, end) HIP event pairs around the encoder launches
        self.time_trunk = False

    # ---- helpers ------------------------------------------------------------------------------
    @property
    def feat(self) -> torch.Tensor:
        """[T+1, N, S*S, C] view for tests / inspection (concatenates the slices)."""
        return self.slices[0].feat if self.ns == 1 else torch.cat([sl.feat for sl in self.slices], dim=1)

    @property
    def feat2(self) -> Optional[torch.Tensor]:
        """The depth tower's features, laid out as ``feat`` (``depth=True``; else None)."""
        if not self.dual:
            return None
        return self.slices[0].feat2 if self.ns == 1 else torch.cat([sl.feat2 for sl in self.slices], dim=1)

    def _f2(self, sl, t: int):
        return sl.feat2[t] if self.dual else None

    def _observe(self, actions_host=None):
        """env.step: the next RGB batch and the second input that goes with it (depth frames / goal-state views; else None)."""
        rgb = self.env.observe(actions_host) if actions_host is not None else self.env.observe()
        return rgb, (self.env.observe_second() if self._has_second else None)

    @property
    def enc_streams(self):
        return [sl.stream for sl in self.slices if sl.stream is not None]

    def _on(self, sl):
        return torch.cuda.stream(sl.stream) if sl.stream is not None else _NullCtx()

    def _fork(self):
        if self.ns > 1:
            cur = torch.cuda.current_stream()
            for sl in self.slices:
                sl.stream.wait_stream(cur)

    def _join(self):
        if self.ns > 1:
            cur = torch.cuda.current_stream()
            for sl in self.slices:
                cur.wait_stream(sl.stream)

    # ---- HOT LOOP A ---------------------------------------------------------------------------
    def _encode_slice(self, sl, rgb: torch.Tensor, t: int, dep: Optional[torch.Tensor] = None):
        src = rgb[sl.o:sl.o + sl.n]
        if self.env.host:
            # H2D of this slice's frames on its copy stream, overlapping whatever the other slice is computing; the
            # staging buffer is reused only after the encoder launch that read it two steps ago has finished
            i = sl.k & 1
            sl.k += 1
            cur = torch.cuda.current_stream()
            with torch.cuda.stream(sl.copy_stream):
                if sl.consumed[i] is not None:
                    sl.copy_stream.wait_event(sl.consumed[i])
                sl.stage[i].copy_(src, non_blocking=True)
                sl.copied[i].record(sl.copy_stream)
            cur.wait_event(sl.copied[i])
            src = sl.stage[i]
        timed = self.time_trunk
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream())
        if self._embed and self.depth:
            # the pooled RGB-D agent: both frames of every pair through the plan in one pass, the two maps summed and average-pooled
            # straight into the rollout slice (the depth wire form is synthetic.normalize_depth: scale 1, shift 0)
            sl.enc.embed_rgbd(src, dep[sl.o:sl.o + sl.n], sl.feat[t].view(sl.n, self.C))
        elif self._embed == "cls":
            sl.enc.embed_cls(src, sl.feat[t].view(sl.n, self.C))      # the class embedding straight into the rollout slice
        elif self._embed:
            (sl.enc.forward_u8 if src.dtype == torch.uint8 else sl.enc.forward)(src, sl.trunk_out)
            if self._embed == "attnpool":
                sl.pool.forward(sl.trunk_out, sl.feat[t].view(sl.n, self.C))     # AttentionPool2d -> rollout slice
            else:                                                               # AdaptiveAvgPool2d(1) -> rollout slice
                _lib.check(self.lib.ec_spatial_mean_bf16(sl.trunk_out.data_ptr(), sl.feat[t].data_ptr(), sl.n, self.trunk_S * self.trunk_S,
                                                         self.trunk_C, _lib.stream_ptr()), "ec_spatial_mean_bf16")
        elif self.encoder in ("rn50", "rn50x16") or self.encoder in IMAGENET_ENCODERS:
            # the last conv writes straight into the rollout slice
            (sl.enc.forward_u8 if src.dtype == torch.uint8 else sl.enc.forward)(src, sl.feat[t])
            if self.two_view_net:   # the goal-state view: the same handle, a second call behind the first on this stream (two calls, not
                g2 = dep[sl.o:sl.o + sl.n]     # one over the stacked 2n frames: the frames of a slice are not contiguous with their goal views)
                (sl.enc.forward_u8 if g2.dtype == torch.uint8 else sl.enc.forward)(g2, sl.feat2[t])
            elif self.dual:    # the depth tower: the same handle on the one-channel batch, behind the RGB tower on this stream
                sl.enc.forward_depth(dep[sl.o:sl.o + sl.n], sl.feat2[t])
        else:
            sl.enc.forward(src, sl.tok)
            sl.feat[t].copy_(sl.tok[:, 1:, :])        # drop CLS: [n,49,768] channels-last rows
        if timed:
            e1.record(torch.cuda.current_stream())
            self.trunk_events.append((e0, e1))
        if self.env.host:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            sl.consumed[i] = ev

    # ---- parameters ---------------------------------------------------------------------------
    def invalidate_act_tables(self):
        """The act workspaces cache weight-derived tables (the goal-embedding table E1, the re-ordered weight_ih).  Call
        this after ANY write to ``self.params`` that does not go through ``update()`` (checkpoint restore, parameter
        broadcast, an external optimiser)."""
        for sl in self.slices:
            sl.act_tables_valid = False

    def set_params(self, flat: torch.Tensor):
        """Replace the flat parameter vector (e.g. a restored checkpoint) and drop everything derived from it."""
        self.params.copy_(flat.to(self.params.device, self.params.dtype).view_as(self.params))
        self.invalidate_act_tables()


class Worker(_SlicedActor):
    """One DD-PPO worker.  The actor batch is processed as ``n_slices`` independent slices (default 2), each with its
    own HIP stream, encoder handle, rollout feature buffer ``[T+1, n, S*S, C]``, policy workspaces and gradient
    bucket.  Slices only meet at the GAE/advantage normalisation and at the gradient sum, so the HBM-bound and
    MFMA-bound launches of one slice overlap the small / latency-bound launches (policy act step, GRU recurrence)
    of the other.  Per-actor arithmetic does not depend on the slicing (tests assert identical features/actions)."""

    def __init__(self, n_actors: int, T: int = 128, device="cuda:0", seed: int = 0, rank: int = 0, world: int = 1,
                 update_repeats: int = 4, lr: float = 3e-4, max_grad_norm: float = 0.5, gamma: float = 0.99,
                 tau: float = 0.95, encoder_sd=None, policy_sd=None, lr_total_steps: int = 300_000_000,
                 encoder_chunk: int = 0, encoder: str = "rn50", encoder_streams: int = 2, frames_u8: bool = False,
                 frames_host: bool = False, zeroshot: bool = False, text_sd=None, goal_tokens=None,
                 num_mini_batch: int = 1, sync_actions: bool = False, force_allreduce: bool = False,
                 overlap_allreduce: bool = True, goal_in: int = 0, num_actions: int = 6, track_episodes: bool = False,
                 nav_metrics: bool = False, depth: bool = False, loss: str = "ppo", il_weight: float = 1.0,
                 teacher_forcing=None, prev_actions: int = 0, prev_action_null_token: bool = True, rnn_type: str = "GRU",
                 rnn_layers: int = 1, hidden: int = 512, net: str = "goal_encoder", pooling: str = "attnpool", sensors=(),
                 goal_ids: bool = True):
        """``net="two_view"``: the rearrangement agent ([U] ai2thor-rearrangement ``ResNetRearrangeActorCriticRNN``, restated, parity
        unpinned; ``PolicyHandle.two_view``) -- the env also serves the goal-state view of every actor and step
        (``SyntheticEnv(goal_view=True)``), every slice's trunk handle encodes it behind the current view into ``feat2``, and the
        trainable attention-pooled front reads both maps.  No goal input.  Works with every ``loss``, teacher forcing, up to 256
        actions, both cells, ``rnn_layers``, ``prev_actions`` up to 512 (upstream's width is ``hidden``), ``num_mini_batch``,
        ``sync_actions``, ``frames_u8`` and checkpoints; ``ValueError`` (``check_net``) with ``depth``, ``zeroshot``, ``goal_in``,
        ``sensors``, ``goal_ids=False``, ``pooling=``, ``encoder="vit"``, ``frames_host``.

        ``net="pooled"``: the Habitat DD-PPO net ([U] habitat-lab ``PointNavResNetNet``, restated, parity unpinned;
        ``PolicyHandle.pooled``) -- the frozen tower pooled to ONE vector per frame (``pooling="attnpool"``: CLIP's attention pool,
        D = 1024, ``encoder="rn50"``; ``"avgpool"``: ``ec_spatial_mean_bf16`` over the trunk output, D = its channels, also on the
        ImageNet towers), ``visual_fc``, the goal id (``goal_ids``) and / or the env's float ``sensors=(k_1, ...)``, the previous
        action, the recurrent core.  The rollout buffer is fp32 ``[T + 1, n, 1, D]``.  Every ``loss`` mode, teacher forcing, up to
        256 actions, ``prev_actions``, ``rnn_type``, ``rnn_layers``, ``num_mini_batch``, ``sync_actions`` and checkpoints work; a
        checkpoint of another net is refused by tensor name.  ``ValueError`` before any allocation with ``zeroshot``,
        ``goal_in``, ``encoder="vit"`` with ``"attnpool"`` / ``"avgpool"``, or ``pooling="attnpool"`` on an ImageNet tower.

        ``net="pooled", encoder="vit", pooling="cls"``: the same net over the ViT's class embedding ([U] ``ClipViTPreprocessor``
        with ``class_emb_only``: token 0 after ``resblocks[:-1]``; the pairing with the pooled net is this project's).  One
        ``ViTEmbedder.embed_cls`` call per slice and env step writes fp32 ``[n, D]`` straight into the rollout slice: no token
        buffer, D floats per frame whatever the token count, and an ``encoder_sd`` of ViT-B/16 or ViT-L/14 geometry works (heads =
        D / 64).  ``pooling="cls"`` with any other encoder is a ``ValueError``.

        ``net="pooled", pooling="avgpool", depth=True`` (``encoder="rn50"``): the same net on RGB-D frames
        (readme_files/baselines_habitat.md:75; [U] habitat branch ``ResNetCLIPEncoder`` with rgb and depth, restated, parity
        unpinned) -- the embedding is ``adaptive_avg_pool2d(trunk(rgb) + trunk(depth), 1)``, D = 2048, one
        ``RN50Trunk.embed_rgbd`` call per slice and env step that runs both frames of every pair through the trunk in ONE pass.
        ``feat2`` is None and the rollout buffer is the RGB avgpool net's; ``frames_u8`` (uint8 RGB, fp32 depth), both cells,
        1..4 layers and ``prev_actions`` work.  A checkpoint has exactly the RGB avgpool net's tensors, so it loads into
        ``Worker(net="pooled", pooling="avgpool")`` with or without ``depth``.  The depth frames arrive as
        ``synthetic.normalize_depth`` serves them (upstream quantises depth to uint8 and applies CLIP's RGB mean / std: a
        deviation).  ``ValueError`` with ``pooling="attnpool"`` (upstream removes the attention pool there), an
        ImageNet tower, ``frames_host`` or ``zeroshot``.

        ``hidden``: the recurrent width ([U] ``hidden_size``; 512 in every published config).

        ``rnn_layers=L`` (1..4; [U] RNNStateEncoder ``num_layers``, 2 in the Habitat DD-PPO policies): the recurrent memory is
        ``[N, L * SW]`` rows, layer-major (``policy.memory_to_state`` converts upstream's); a checkpoint carries the upper
        layers' tensors ``state_encoder.rnn.*_l{k}`` and one of another depth is refused by tensor name; their gradients are
        all-reduced with the sections outside ``recurrent_section()``.  ``ValueError`` with ``depth=True`` or ``zeroshot=True``.

        ``rnn_type``: "GRU" (default) or "LSTM" ([U] RNNStateEncoder ``rnn_type``; the Habitat DD-PPO policies) -- the
        recurrent memory ``h`` / ``h_next`` / ``h_start`` is then ``[N, 2 * hidden]`` rows ``[h | c]``, checkpoints carry the
        ``4 * hidden``-row recurrent tensors under the same names.  ``ValueError`` with ``depth=True`` or ``zeroshot=True``.

        ``loss``: what a rollout is trained on -- "ppo" (GAE, then the PPO loss: the default), "imitation" (the expert
        cross-entropy of [U] AllenAct's ``Imitation`` loss on the env's expert actions; no GAE launch) or "ppo+imitation"
        (``ppo_total + il_weight * imitation``: the PPO call writes d(total)/d(hv), the imitation call adds its term).
        ``il_weight`` is the imitation term's loss weight in both.  ``teacher_forcing``: None, or a callable of ``total_steps``
        (``imitation.LinearDecay`` / ``StepwiseLinearDecay``) giving the probability p with which a step that has an expert
        action TAKES it ([U] ``TeacherForcingDistr``; DAgger is a p that decays from 1): evaluated once per rollout, at the
        rollout's first ``total_steps``; one small launch behind every sampling act step while p > 0, none otherwise.  With
        the defaults nothing of this runs and the env builds no expert.

        ``prev_actions=E > 0``: the agent also conditions on its previous action ([U] VisualNavActorCritic ``add_prev_actions``,
        ``action_embed_size=E``; Habitat's ``prev_action_embedding``, E = 32) -- ``PolicyHandle(prev_action_dims=E)``, one more
        parameter tensor.  ``prev_action_null_token`` (default True, Habitat's rule): an episode's first step reads the null
        row.  The rollout's ``actions`` are rows 1..T of a ``[T + 1, N]`` buffer whose row ``t`` is step ``t``'s previous action
        (row 0: the previous rollout's last), so the act step's selection and the teacher forcing write where the next step
        reads -- no copy.  Works with every ``loss``, teacher forcing, ``goal_in``, up to 256 actions, ``sync_actions``;
        ``ValueError`` with ``depth=True`` or ``zeroshot=True``.  The imitation normaliser (the number of steps with an
        expert action in a minibatch range) is rank-local, as the advantage normalisation is.

        ``depth=True``: the RGB-D agent (readme_files/baselines_habitat.md:75; [U] a second ClipResNetPreprocessor on the
        depth sensor feeding ResnetDualTensorGoalEncoder): the env also serves one-channel depth frames, every slice's trunk
        runs twice per env step (RGB, then depth through the one-channel stem) into ``feat`` / ``feat2``, and the policy is
        ``PolicyHandle(dual=1)``.  Rollout feature storage doubles.  Only with ``encoder`` "rn50" / "rn50x16", goal ids and
        device-resident frames.

        ``track_episodes=True``: ``compute_returns()`` also folds the rollout's completed episodes into an ``EpisodeTracker``
        (one more launch per iteration; ``episode_info()`` reads the means AllenAct logs every rollout).  Default off.
        ``nav_metrics=True`` (with ``track_episodes``): the tracker is a ``NavEpisodeTracker`` on a ``NavSyntheticEnv`` and
        ``episode_info()`` also carries ``spl``, ``soft_spl``, ``dist_to_goal``, ``path_length``, ``no_path``.

        ``goal_in > 0``: the PointNav agent ([U] ResnetTensorPointNavActorCritic) -- the goal of a frame is ``goal_in``
        floats (GPS + compass: distance, bearing), ``num_actions`` is 4 there; ``goal_in=0`` is the ObjectNav agent.

        ``zeroshot=True`` (BASELINE config 5, readme_files/zeroshot_objectnav.md): the observation is the CLIP image
        EMBEDDING (RN50 trunk + AttentionPool2d, 1024-d), the goal is the frozen CLIP text embedding of its prompt
        (text tower run once -> [12, 1024] table) and the policy is the fusion=1 variant (GRU + heads trainable)."""
        self._configure(encoder, net, pooling, sensors, goal_ids, goal_in, depth, zeroshot, num_actions, prev_actions,
                        prev_action_null_token, rnn_type, rnn_layers, hidden, frames_host=frames_host)
        self._text_sd, self._goal_tokens = text_sd, goal_tokens
        self.track_episodes = track_episodes
        if nav_metrics and not track_episodes:
            raise ValueError("Worker(nav_metrics=True) needs track_episodes=True")
        self.nav_metrics = nav_metrics
        if loss not in ("ppo", "imitation", "ppo+imitation"):
            raise ValueError(f"Worker(loss={loss!r}): one of 'ppo', 'imitation', 'ppo+imitation'")
        if teacher_forcing is not None and not callable(teacher_forcing):
            raise ValueError("Worker(teacher_forcing=...): None or a callable of total_steps")
        self.loss_mode, self.il_weight, self.teacher_forcing = loss, float(il_weight), teacher_forcing
        self._ppo, self._il = loss != "imitation", loss != "ppo"
        self._tf_p = 0.0                                    # this rollout's forcing probability (collect_rollout sets it)
        # sync_actions: the action-synchronous order of a real vectorised env ([U] VectorSampledTasks.step(actions)): every
        # env step the sampled actions of ALL actors are copied to the host and waited for before observe() serves the next
        # frames.  Default off: the synthetic env does not read the actions and the host issues ahead.
        self.sync_actions = sync_actions
        # force_allreduce: run the flat-bucket collective also at world size 1 (RCCL first-contact check on a 1-GPU box)
        self.force_allreduce = force_allreduce
        # overlap_allreduce (when there is a collective at all): the GRU + heads section of the flat bucket (92 % of its bytes,
        # final first: ec_policy_backward3) is summed over ranks on a communication stream UNDER the rest of the backward;
        # only the goal encoder's 1.1 MB is reduced after it.  False: one 13.9-MB all-reduce after the backward
        self.overlap_allreduce = overlap_allreduce
        # [U] allenact RolloutStorage.recurrent_generator(num_mini_batch): contiguous sampler ranges, shuffled order
        assert 1 <= num_mini_batch <= n_actors, "num_mini_batch must not exceed the number of samplers"
        self.num_mini_batch = num_mini_batch
        # ONE shuffle stream for all ranks: every rank visits the same minibatch range at the same optimiser step, so the
        # SUM all-reduce with the fixed 1/world scale is the global minibatch mean also when N % num_mini_batch != 0
        # (ranges of different sizes) -- with per-rank streams it would be a mean of differently-sized means
        self._mb_rng = random.Random(seed)                  # (`seed` is the job's seed: identical on every rank)
        self.dev = self.device = torch.device(device)
        if self.dev.index is None:
            self.dev = self.device = torch.device("cuda", torch.cuda.current_device())
        check_job_seed(seed, world, device=self.dev)        # ... which is ENFORCED when a process group is up (on THIS worker's GPU)
        # every rank's actor count: the gradient scale is local / GLOBAL minibatch size ([U] backprop_step), and the global size
        # is the sum over the ranks -- shards need not be equal (dist.shard_actors(10, r, 3) = 4, 3, 3)
        self.shard_counts = gather_actor_counts(n_actors, world, device=self.dev)
        assert all(num_mini_batch <= c for c in self.shard_counts), "num_mini_batch must not exceed the smallest shard"
        self._mb_global = global_minibatch_sizes(self.shard_counts, num_mini_batch)
        self._init(n_actors, T, seed, rank, world, update_repeats, lr, max_grad_norm, gamma, tau, encoder_sd, policy_sd,
                   lr_total_steps, encoder_chunk, encoder, encoder_streams, frames_u8, frames_host)

    @_lib.on_device
    def _init(self, n_actors, T, seed, rank, world, update_repeats, lr, max_grad_norm, gamma, tau, encoder_sd, policy_sd,
              lr_total_steps, encoder_chunk, encoder, encoder_streams, frames_u8, frames_host=False):
        self.N, self.T, self.rank, self.world = n_actors, T, rank, world
        self.update_repeats, self.gamma, self.tau = update_repeats, gamma, tau
        self.base_lr, self.lr_total_steps = lr, lr_total_steps
        d = self.dev
        encs, pools = self._build_model(n_actors, encoder, encoder_sd, policy_sd, encoder_chunk, encoder_streams)
        ns = self.ns
        self.grads = torch.zeros_like(self.params)
        self.rec = self.policy.recurrent_section()          # GRU + heads: the part of the bucket whose gradients are final first
        self.opt = FlatAdam(self.params, lr=lr, max_grad_norm=max_grad_norm)
        N = n_actors
        # [T, N] rollout scalars (global; tiny)
        if self.prev_action_dims:     # row t: step t's previous action; rows 1..T ARE the rollout's actions, row 0 the last rollout's last
            self.prev_actions = torch.zeros((T + 1, N), dtype=torch.int64, device=d)
            self.actions = self.prev_actions[1:]
        else:
            self.prev_actions = None
            self.actions = torch.zeros((T, N), dtype=torch.int64, device=d)
        self.logp = torch.zeros((T, N), dtype=torch.float32, device=d)
        self.values = torch.zeros((T + 1, N), dtype=torch.float32, device=d)
        self.returns = torch.zeros((T + 1, N), dtype=torch.float32, device=d)
        self.adv = torch.zeros((T, N), dtype=torch.float32, device=d)
        self.nadv = torch.zeros((T, N), dtype=torch.float32, device=d)
        self.h_start = torch.zeros((N, self.SW), dtype=torch.float32, device=d)
        self.h = torch.zeros((N, self.SW), dtype=torch.float32, device=d)
        self.h_next = torch.zeros((N, self.SW), dtype=torch.float32, device=d)
        self.hv_act = torch.empty((N, self.A + 1), dtype=torch.float32, device=d)
        self.stats = torch.zeros(2, dtype=torch.float64, device=d)
        self.sums = torch.zeros(4, dtype=torch.float64, device=d)
        env_cls, ekw = self._env_recipe(expert=self._il or self.teacher_forcing is not None)
        self.env = env_cls(N, T, d, seed=1000 + rank, frames_u8=frames_u8, host=frames_host, **ekw)
        self.episodes = self._episode_tracker() if self.track_episodes else None
        self._build_slices(n_actors, encs, pools, T + 1, 1 if (world > 1 or self.force_allreduce) else 0, frames_host)
        if self.comm_stream is None:
            self.comm_stream = torch.cuda.Stream(device=d)
        for sl in self.slices:      # the learn pass's share of a slice
            sl.ws_learn = torch.empty(self.policy.workspace_bytes(T, sl.n, True), dtype=torch.uint8, device=d)
            sl.hv = torch.empty((T * sl.n, self.A + 1), dtype=torch.float32, device=d)
            sl.dhv = torch.empty_like(sl.hv)
            sl.grads = self.grads if ns == 1 else torch.zeros_like(self.params)
            sl.rec_ready = torch.cuda.Event()
            sl.rec_ready.record()          # (torch creates the hipEvent_t at the first record: the library needs the handle)
            sl.sums = torch.zeros(4, dtype=torch.float64, device=d)
            sl.cols = None             # this rollout's [T, n, ...] columns of the slice (update() fills them)
            sl.feat_mb = sl.feat2_mb = None      # staging of the feature columns of a partial range (gather() makes them)
            # more than 16 actions: the wide loss kernel's partial-sum scratch, one per slice stream as for imitation
            sl.ppo_scratch = ppo_wide_scratch(d) if (self._ppo and self.A > PPO_NARROW_MAX_A) else None
            if self._il:      # the imitation loss's sums and partial-sum scratch: one per slice stream
                sl.il_sums = torch.zeros(3, dtype=torch.float64, device=d)
                sl.il_scratch = imitation_scratch(d)
        if self._il:          # one normaliser per minibatch range (update() fills them once per rollout)
            self._il_denoms = torch.zeros(self.num_mini_batch, dtype=torch.float64, device=d)
        self.seed = seed + 7919 * rank
        self.total_steps = 0
        self.iter = 0
        self.update_events: List = []            # (start, end) HIP event pairs around the update phase (GAE excluded), one pair per timed iteration
        # first observation of the first rollout
        rgb, dep = self._observe()
        for sl in self.slices:
            self._encode_slice(sl, rgb, 0, dep)
        torch.cuda.synchronize(d)

    # ---- HOT LOOP A ---------------------------------------------------------------------------
    def _act_slice(self, sl, t: int, sample: bool = True):
        """Policy act step (T=1, no grad) for the slice's actors on the current stream."""
        o, n, sp = sl.o, sl.n, _lib.stream_ptr()
        rs = slice(o, o + n)
        h_in, h_out = (self.h, self.h_next) if (t & 1) == 0 else (self.h_next, self.h)   # ping-pong by step parity
        pa = self.prev_actions[t][rs] if self.prev_action_dims else None                  # (the bootstrap step reads row T)
        goal = self.env.goals[t][rs] if self._has_goal else None            # (what the agent description decided: plain attributes,
        sens = self.env.sensors[t][rs] if self._has_sensors else None       #  no call on this host chain)
        if sample and self._act_fused:
            # forward + CategoricalDistr.sample / log_prob in one call: the heads launch samples (ec_policy_act, one launch less)
            self.policy.act(self.params, sl.feat[t], goal, h_in[rs], self.env.masks[t][rs], n, sl.ws_act,
                            self.hv_act[rs], h_out[rs], self.actions[t][rs], self.logp[t][rs], self.values[t][rs], self.seed,
                            self.iter * (self.T + 1) + t, o, reuse_tables=sl.act_tables_valid, feat2=self._f2(sl, t), prev_actions=pa,
                            sensors=sens)
            sl.act_tables_valid = True
            self._teacher_force_slice(sl, t)
            return
        if sample and self._act_wide:
            # the same for 8 to 256 actions (ec_policy_act_ex): the wide heads launch samples and, while p > 0, forces
            tf = self._tf_p > 0.0
            self.policy.act_ex(self.params, sl.feat[t], goal, h_in[rs], self.env.masks[t][rs], n, sl.ws_act,
                               self.hv_act[rs], h_out[rs], self.actions[t][rs], self.logp[t][rs], self.values[t][rs], self.seed,
                               self.iter * (self.T + 1) + t, o, reuse_tables=sl.act_tables_valid, feat2=self._f2(sl, t),
                               expert_actions=self.env.expert_actions[t][rs] if tf else None,
                               expert_mask=self.env.expert_mask[t][rs] if tf else None, force_p=self._tf_p if tf else 0.0,
                               prev_actions=pa, sensors=sens)
            sl.act_tables_valid = True
            return
        self.policy.forward(self.params, sl.feat[t], goal, h_in[rs], self.env.masks[t][rs], 1, n,
                            sl.ws_act, hv=self.hv_act[rs], h_final=h_out[rs], for_backward=False,
                            reuse_tables=sl.act_tables_valid, feat2=self._f2(sl, t), prev_actions=pa, sensors=sens)   # (E1 depends on the parameters only)
        sl.act_tables_valid = True
        if sample:
            _lib.check(self.lib.ec_sample_actions(self.hv_act[rs].data_ptr(), self.actions[t][rs].data_ptr(),
                                                  self.logp[t][rs].data_ptr(), self.values[t][rs].data_ptr(), n, self.A,
                                                  self.seed, self.iter * (self.T + 1) + t, o, sp), "ec_sample_actions")
            self._teacher_force_slice(sl, t)
        else:   # bootstrap value of the last observation; memory is NOT advanced
            self.values[t][rs].copy_(self.hv_act[rs, self.A])

    def _teacher_force_slice(self, sl, t: int):
        """[U] TeacherForcingDistr behind a sampling act step: with this rollout's probability p, a step that has an expert
        action takes it (action and log-prob; ec_teacher_force) -- on the slice's stream, keyed like the sampler.  No launch
        while p is 0."""
        if self._tf_p <= 0.0:
            return
        rs = slice(sl.o, sl.o + sl.n)
        _lib.check(self.lib.ec_teacher_force(self.hv_act[rs].data_ptr(), self.env.expert_actions[t][rs].data_ptr(),
                                             self.env.expert_mask[t][rs].data_ptr(), self._tf_p,
                                             self.actions[t][rs].data_ptr(), self.logp[t][rs].data_ptr(), sl.n, self.A,
                                             self.seed, self.iter * (self.T + 1) + t, sl.o, _lib.stream_ptr()),
                   "ec_teacher_force")

    @_lib.on_device
    def collect_rollout(self):
        T = self.T
        self.h_start.copy_(self.h)
        if self.teacher_forcing is not None:      # p of this rollout: the schedule at the rollout's first total_steps
            self._tf_p = float(self.teacher_forcing(self.total_steps))
            if not 0.0 <= self._tf_p <= 1.0:
                raise ValueError(f"teacher_forcing({self.total_steps}) = {self._tf_p}: a probability is expected")
        self._fork()
        if self.sync_actions:
            return self._collect_rollout_sync()
        for t in range(T):
            rgb, dep = self._observe()    # env.step(actions[t]) happens here in the real system (fp32 NHWC frames)
            for sl in self.slices:
                with self._on(sl):
                    self._act_slice(sl, t)
                    self._encode_slice(sl, rgb, t + 1, dep)
        for sl in self.slices:
            with self._on(sl):
                self._act_slice(sl, T, sample=False)
        self._join()
        if (T & 1) == 1:   # after an odd number of advancing steps the live memory sits in h_next
            self.h, self.h_next = self.h_next, self.h

    def _collect_rollout_sync(self):
        """The action-synchronous orders: one host round trip per env step sits between act(t) and encode(t+1), as in the
        real engine.

        ``sync_actions=True`` ("all"): ONE vectorised env for all actors ([U] ``VectorSampledTasks.step(actions)``): act(t)
        on every slice -> actions[t] D2H, WAITED FOR -> env.step -> encode(t+1) on every slice.  The slices then run in
        lock step and the chip idles over the round trip only: 0.99 x the free-running rate at 256 actors (measured round 5;
        the 0.77 x of rounds 3-4 was two slice streams sharing one hardware queue: _lib.concurrent_streams).

        ``sync_actions="slice"``: one vectorised env PER SLICE (two ``VectorSampledTasks`` groups): the host waits for the
        actions of slice s only, steps that slice's env and issues its encode(t+1) + act(t+1) -- while the other slice's
        encoder is still running.  Same per-actor arithmetic and the same number of round trips per actor, but the two
        slices stay out of phase as they do in the free-running order."""
        T = self.T
        if getattr(self, "_actions_host", None) is None:
            self._actions_host = torch.empty((self.N,), dtype=torch.int64).pin_memory()
        k0 = self.env._k

        def d2h(sl, t):
            self._actions_host[sl.o:sl.o + sl.n].copy_(self.actions[t][sl.o:sl.o + sl.n], non_blocking=True)

        def wait(sl):
            (sl.stream if sl.stream is not None else torch.cuda.current_stream()).synchronize()

        if self.sync_actions == "slice":
            for sl in self.slices:
                with self._on(sl):
                    self._act_slice(sl, 0)
                    d2h(sl, 0)
            for t in range(T):
                for sl in self.slices:
                    wait(sl)                                                 # this slice's actions[t] are on the host
                    rgb = self.env.observe_at(k0 + t, self._actions_host)   # env.step of this slice's samplers
                    dep = self.env.observe_second_at(k0 + t) if self._has_second else None
                    with self._on(sl):
                        self._encode_slice(sl, rgb, t + 1, dep)
                        if t + 1 < T:
                            self._act_slice(sl, t + 1)
                            d2h(sl, t + 1)
                        else:
                            self._act_slice(sl, T, sample=False)
            self.env._k = k0 + T
        else:
            for t in range(T):
                for sl in self.slices:
                    with self._on(sl):
                        self._act_slice(sl, t)
                        d2h(sl, t)
                for sl in self.slices:
                    wait(sl)
                rgb, dep = self._observe(self._actions_host)        # env.step(actions[t])
                for sl in self.slices:
                    with self._on(sl):
                        self._encode_slice(sl, rgb, t + 1, dep)
            for sl in self.slices:
                with self._on(sl):
                    self._act_slice(sl, T, sample=False)
        self._join()
        if (T & 1) == 1:
            self.h, self.h_next = self.h_next, self.h

    @_lib.on_device
    def compute_returns(self):
        if self._ppo:         # (pure imitation reads neither returns nor advantages: no GAE launch)
            _lib.check(self.lib.ec_gae(self.env.rewards.data_ptr(), self.values.data_ptr(), self.env.masks.data_ptr(),
                                       self.returns.data_ptr(), self.adv.data_ptr(), self.nadv.data_ptr(),
                                       self.stats.data_ptr(), self.T, self.N, self.gamma, self.tau, 1e-5,
                                       _lib.stream_ptr()), "ec_gae")
        if self.episodes is not None:
            self._update_episodes()

    # ---- HOT LOOP B ---------------------------------------------------------------------------
    def _rollout_columns(self):
        """name -> the [T (+ 1), N, ...] storage of every per-step column THIS agent's learn pass reads beside the features."""
        cols = dict(masks=self.env.masks, actions=self.actions, logp=self.logp, old_values=self.values, returns=self.returns,
                    advantages=self.nadv)
        if self._has_goal:            # int64 ids [., N], or (coordinate goals) f32 [., N, goal_in]
            cols["goal"] = self.env.goals
        if self._has_sensors:         # the pooled net's sensor rows [., N, K]
            cols["sensors"] = self.env.sensors
        if self._il:
            cols.update(expert_actions=self.env.expert_actions, expert_mask=self.env.expert_mask)
        if self.prev_action_dims:     # rows 0..T-1: every step's previous action
            cols["prev_actions"] = self.prev_actions
        return cols

    def _gather_columns(self):
        """Every slice's table of columns: contiguous [T, n, ...] copies of its actors' part of the rollout storage (once per
        iteration)."""
        cols = self._rollout_columns()
        for sl in self.slices:
            sl.cols = {name: x[:self.T, sl.o:sl.o + sl.n].contiguous() for name, x in cols.items()}

    def minibatch_ranges(self):
        """[U] allenact ``RolloutStorage.recurrent_generator``: the samplers (actors) are cut at
        ``round(linspace(0, N, num_mini_batch + 1))`` into contiguous ranges which are visited in a shuffled order;
        every range keeps its full T-step sequences (the GRU needs them)."""
        inds = minibatch_bounds(self.N, self.num_mini_batch)      # == np.round(np.linspace(0, N, M + 1))
        # (s0, s1, samplers of this range over ALL ranks); the shuffle permutation depends on the list's length only
        pairs = [(s0, s1, g) for s0, s1, g in zip(inds[:-1], inds[1:], self._mb_global)]
        self._mb_rng.shuffle(pairs)
        return pairs

    def _max_partial_range(self, sl) -> int:
        inds = minibatch_bounds(self.N, self.num_mini_batch)
        best = 1
        for s0, s1 in zip(inds[:-1], inds[1:]):
            a, b = max(s0, sl.o) - sl.o, min(s1, sl.o + sl.n) - sl.o
            if b > a and not (a == 0 and b == sl.n):
                best = max(best, b - a)
        return best

    def gather(self, sl, a: int, b: int) -> Dict[str, torch.Tensor]:
        """The learn batch of actors [a, b) of slice ``sl`` (slice-local indices): {column: contiguous [T * (b - a), ...] rows} over
        ``feat``, ``feat2`` (an agent with a second feature buffer) and the slice's table (``_rollout_columns``).  The whole slice is
        used in place; a partial range is a copy -- of the features through the staging buffers ``sl.feat_mb`` / ``sl.feat2_mb``,
        allocated on first use and sized to the largest PARTIAL range, not the whole slice."""
        T, m, S2 = self.T, b - a, self.S * self.S
        whole = a == 0 and b == sl.n
        out = {}
        for name, src in (("feat", sl.feat), ("feat2", sl.feat2)):
            if src is None:
                continue
            if whole:
                out[name] = src[:T].view(T * m, S2, self.C)
                continue
            stage = getattr(sl, name + "_mb")
            if stage is None:
                stage = torch.empty((T, self._max_partial_range(sl), S2, self.C), dtype=src.dtype, device=self.dev)
                setattr(sl, name + "_mb", stage)
            fm = stage.view(-1)[:T * m * S2 * self.C].view(T, m, S2, self.C)
            fm.copy_(src[:T, a:b])
            out[name] = fm.view(T * m, S2, self.C)
        for name, col in sl.cols.items():      # [T, n, ...] -> [T * m, ...]
            out[name] = (col if whole else col[:, a:b].contiguous()).view((T * m,) + col.shape[2:])
        return out

    def _expert_counts(self) -> Dict[tuple, torch.Tensor]:
        """The imitation normaliser of every minibatch range -- the number of this rollout's steps that have an expert action
        among the range's samplers (rank-local) -- once per rollout, on the current stream: {(s0, s1): float64 [1] view}."""
        inds = minibatch_bounds(self.N, self.num_mini_batch)
        out = {}
        for j, (s0, s1) in enumerate(zip(inds[:-1], inds[1:])):
            out[(s0, s1)] = self._il_denoms[j:j + 1]
            _lib.check(self.lib.ec_expert_count(self.env.expert_mask.data_ptr(), self.T, self.N, s0, s1,
                                                out[(s0, s1)].data_ptr(), _lib.stream_ptr()), "ec_expert_count")
        return out

    def _sum_parts(self, parts, sec: slice):
        """self.grads[sec] = sum of the slices' gradient buckets over ``sec`` (one slice: its bucket IS self.grads)."""
        if self.ns == 1:
            return
        if len(parts) == 1:
            self.grads[sec].copy_(parts[0][0].grads[sec])
            return
        torch.add(parts[0][0].grads[sec], parts[1][0].grads[sec], out=self.grads[sec])
        for (sl, _, _) in parts[2:]:
            self.grads[sec].add_(sl.grads[sec])

    def _other_sections(self):
        """What ``self.rec`` leaves of the flat bucket (the goal encoder's tensors; two pieces with the dual encoder)."""
        n = self.grads.numel()
        return [sec for sec in (slice(0, self.rec.start), slice(self.rec.stop, n)) if sec.stop > sec.start]

    @_lib.on_device
    def update(self):
        T = self.T
        collective = collective_active(self.world, self.force_allreduce)
        self._gather_columns()
        il_denoms = self._expert_counts() if self._il else None      # (the _fork() below orders the slice streams behind it)
        for _ in range(self.update_repeats):
            for (s0, s1, nmb_global) in self.minibatch_ranges():
                # the minibatch's actors, slice by slice (each part on its slice's stream)
                parts = []
                for sl in self.slices:
                    a, b = max(s0, sl.o) - sl.o, min(s1, sl.o + sl.n) - sl.o
                    if b > a:
                        parts.append((sl, a, b))
                early = collective and self.overlap_allreduce
                if early:                      # (the previous optimiser step read self.grads on the main stream)
                    self.comm_stream.wait_stream(torch.cuda.current_stream())
                self._fork()
                for (sl, a, b) in parts:
                    with self._on(sl):
                        m = b - a
                        g = self.gather(sl, a, b)
                        feat, feat2, masks = g["feat"], g.get("feat2"), g["masks"]
                        hv, dhv = sl.hv[:T * m], sl.dhv[:T * m]
                        # d(total)/d(hv) carries 1/B_part inside the loss kernel: rescale to the mean over the WHOLE
                        # local minibatch (m / nmb), then local_bsize / global_bsize (nmb / nmb_global: the sum of the
                        # ranks' sizes of this range, equal shards or not) for the SUM all-reduce = the global mean gradient
                        grad_scale = m / nmb_global
                        # (staggering the slices -- slice 1's forward starting when slice 0's is done, so that wide GEMMs
                        #  run beside the other slice's GRU recurrence -- was measured in round 3: 53 -> 58 ms per update;
                        #  the step kernels wait for CUs the GEMM workgroups hold)
                        self.policy.forward(self.params, feat, g.get("goal"), self.h_start[sl.o + a:sl.o + b], masks, T, m,
                                            sl.ws_learn, hv=hv, feat2=feat2, prev_actions=g.get("prev_actions"),
                                            sensors=g.get("sensors"))
                        if self._ppo:
                            ppo_loss_raw(hv, g["actions"], g["logp"], g["old_values"], g["returns"], g["advantages"], self.A,
                                         grad_scale=grad_scale, dhv=dhv, sums=sl.sums, scratch=sl.ppo_scratch)
                        if self._il:
                            # the kernel divides by the RANGE's normaliser (shared by the parts), so only local / global
                            # minibatch size is left to apply; after a PPO call the term is added to its dhv
                            imitation_loss_raw(hv, g["expert_actions"], g["expert_mask"], self.A, weight=self.il_weight,
                                               grad_scale=(s1 - s0) / nmb_global, denom=il_denoms[(s0, s1)], dhv=dhv,
                                               sums=sl.il_sums, scratch=sl.il_scratch, accumulate=self._ppo)
                        sl.grads.zero_()
                        self.policy.backward(self.params, feat, masks, T, m, sl.ws_learn, dhv, None, sl.grads, feat2=feat2,
                                             recurrent_ready=sl.rec_ready if early else None)
                if early:
                    # GRU + heads section: summed over the slices and over the ranks on the communication stream, behind the
                    # events the backwards record -- i.e. under the goal encoder's backward (dx GEMM, tail, dW1) of every slice
                    with torch.cuda.stream(self.comm_stream):
                        for (sl, _, _) in parts:
                            self.comm_stream.wait_event(sl.rec_ready)
                        self._sum_parts(parts, self.rec)
                        allreduce_flat(self.grads[self.rec], force=self.force_allreduce)
                self._join()
                self._loss_parts = [(sl, b - a) for (sl, a, b) in parts]
                if early:
                    # the goal encoder's section(s): after the backwards, on the main stream (1.1 MB)
                    for sec in self._other_sections():
                        self._sum_parts(parts, sec)
                        allreduce_flat(self.grads[sec], force=self.force_allreduce)
                    torch.cuda.current_stream().wait_stream(self.comm_stream)
                else:
                    self._sum_parts(parts, slice(0, self.grads.numel()))
                    if collective:
                        allreduce_flat(self.grads, force=self.force_allreduce)   # one flat 13.9 MB bucket over RCCL/xGMI
                self.opt.step(self.grads, lr=linear_decay_lr(self.base_lr, self.total_steps, self.lr_total_steps))
                self.invalidate_act_tables()

    @_lib.on_device
    def after_update(self):
        for sl in self.slices:
            sl.feat[0].copy_(sl.feat[self.T])
            if self.dual:
                sl.feat2[0].copy_(sl.feat2[self.T])
        if self.prev_action_dims:     # the next rollout's first step follows this rollout's last action
            self.prev_actions[0].copy_(self.prev_actions[self.T])
        self.total_steps += self.T * sum(self.shard_counts)
        self.iter += 1

    def iteration(self):
        self.collect_rollout()
        self.compute_returns()
        timed = self.time_trunk          # (bench.py: HIP events around the update phase on the main stream; no host sync)
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.device(self.dev):
                e0.record(torch.cuda.current_stream())
        self.update()
        if timed:
            with torch.cuda.device(self.dev):
                e1.record(torch.cuda.current_stream())
            self.update_events.append((e0, e1))
        self.after_update()

    def episode_info(self) -> Dict[str, float]:
        """``{"episodes", "reward", "reward_std", "ep_length", "success"}`` over the episodes completed so far: the scalars
        [U] AllenAct logs every rollout (``track_episodes=True`` only)."""
        if self.episodes is None:
            raise RuntimeError("Worker(track_episodes=True) keeps the episode metrics")
        return self.episodes.info()

    # ---- checkpoints --------------------------------------------------------------------------
    def save_checkpoint(self, path: str) -> None:
        """``torch.save`` of ``{"model_state_dict", "optimizer_state_dict", "total_steps"}``: the key layout of [U] AllenAct's
        ``exp_...__stage_00__steps_N.pt`` files RESTATED, not pinned against one -- the model's tensors under
        AllenAct's parameter names (``ResnetTensorObjectNavActorCritic.load_state_dict`` takes them), the optimiser as the
        flat Adam moments (``exp_avg``, ``exp_avg_sq``, ``step``) of the flat bucket, not torch's per-parameter state."""
        model = OrderedDict((k, v.detach().cpu().clone()) for k, v in self.policy.views(self.params).items())
        torch.save({"model_state_dict": model,
                    "optimizer_state_dict": {"exp_avg": self.opt.m.cpu(), "exp_avg_sq": self.opt.v.cpu(), "step": self.opt.step_count},
                    "total_steps": self.total_steps}, path)

    def load_checkpoint(self, path: str) -> None:
        """Restore what ``save_checkpoint`` wrote: the parameters (through ``set_params``: the act tables are dropped), the
        Adam moments and step count, and ``total_steps`` (the learning-rate schedule's position).  ``iter`` -- the iteration
        index in the sampling keys ``iter * (T + 1) + t`` -- is set to the number of rollouts ``total_steps`` stands for with
        THIS worker's rollout size, so a resumed worker does not redraw the keys of iteration 0.  Not restored: the
        minibatch shuffle stream (``_mb_rng`` restarts from the seed), the recurrent memory and the env's position -- a
        resumed run continues the optimisation, it is not a bit-for-bit continuation of the uninterrupted one."""
        ck = torch.load(path, map_location="cpu")
        check_model_tensors(self.policy, ck["model_state_dict"], path)
        self.set_params(self.policy.flatten(ck["model_state_dict"], self.dev))
        o = ck["optimizer_state_dict"]
        self.opt.m.copy_(o["exp_avg"].to(self.dev).view_as(self.opt.m))
        self.opt.v.copy_(o["exp_avg_sq"].to(self.dev).view_as(self.opt.v))
        self.opt.step_count = int(o["step"])
        self.total_steps = int(ck["total_steps"])
        self.iter = self.total_steps // (self.T * sum(self.shard_counts))

    def loss_info(self) -> Dict[str, float]:
        parts = getattr(self, "_loss_parts", None) or [(sl, sl.n) for sl in self.slices]   # the last minibatch
        info = {}
        if self._ppo:
            tot = sum(sl.sums for sl, _ in parts)
            s = (tot / (self.T * sum(m for _, m in parts))).tolist()
            info.update({"action": s[0], "value": s[1], "entropy": s[2], "ratio": s[3],
                         "ppo_total": s[0] + 0.5 * s[1] + 0.01 * s[2]})
        if self._il:          # the parts' sums over the steps that have an expert action; divided here, on the host
            nll, cnt, agree = sum(sl.il_sums for sl, _ in parts).tolist()
            info.update({"expert_cross_entropy": nll / max(cnt, 1.0), "expert_agreement": agree / max(cnt, 1.0),
                         "expert_steps": cnt})
        info["grad_norm"] = self.opt.grad_norm()
        return info


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
