"""Evaluation: run a trained agent and read out how well it does.

The reference ends its experiment pages with this step -- ``--eval`` appended to the training command
(readme_files/baselines_robothor_objectnav.md:66-68), ``--run-type eval`` (baselines_habitat.md:89-97), the same config with
``--eval -c $CKPT_PATH`` (zeroshot_objectnav.md:20-27) -- which [U] AllenAct serves with ``OnPolicyInference``: the act loop of
training without storage, loss or optimiser, ``CategoricalDistr.mode()`` or ``sample()`` for the actions, and the finished
tasks' metrics averaged at the end.

``Evaluator`` is hot loop A of ``engine.Worker`` alone, built from the same parts (``engine._SlicedActor``): per slice stream
``act(t)`` then ``encode(t + 1)``.  It allocates no learn workspace, no ``hv`` / ``dhv``, no gradient buckets and no ``[T+1]``
feature storage: each slice keeps a two-entry feature ring.  The episode metrics come from ``episodes.EpisodeTracker``, or with
``nav_metrics=True`` from ``episodes.NavEpisodeTracker``: SPL, SoftSPL, distance to goal, and all of them per goal category --
the success / SPL per object type that readme_files/zeroshot_objectnav.md:20-48 reads from the metrics file of an ``--eval``
run (``write_metrics_json`` / ``scores_by_object_type``).
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .engine import _SlicedActor
from .episodes import category_names, nav_env_tensors


class Evaluator(_SlicedActor):
    """``run(chunks)`` plays ``chunks * T`` env steps of ``n_actors`` actors; ``info()`` returns the episode metrics.

    Chunk ``c``, step ``t`` reads ``env.masks[t]`` / ``env.goals[t]`` and (when sampling) draws with the seed ``seed + 7919 *
    rank`` and the key ``c * (T + 1) + t`` -- what a ``Worker`` with the same arguments uses in iteration ``c``, so with equal
    weights the two take the same actions.  ``deterministic=True`` takes ``CategoricalDistr.mode()`` instead
    (``ec_policy_act_greedy``).  The memory ``h`` carries across chunks.  ``checkpoint=`` is a file of
    ``Worker.save_checkpoint`` (its ``model_state_dict``); otherwise ``policy_sd`` or the seeded stand-in weights.
    ``record=True`` keeps ``actions``, ``logp``, ``values`` ``[chunks*T, N]`` and ``hv`` ``[chunks*T, N, A+1]`` of the last
    ``run`` (tests).  ``env=``: any object with ``SyntheticEnv``'s attributes (``N``, ``T``, ``frames``, ``masks``, ``goals``,
    ``rewards``, ``success``, ``host``, ``observe``); its ``N`` and ``T`` must be the evaluator's.  ``sync_actions=True``: every step's actions are copied to the host and waited for
    before the env serves the next frames (one vectorised env for all actors).  ``nav_metrics=True``: the tracker is a
    ``NavEpisodeTracker`` fed the env's ``step_dist`` / ``start_dist`` / ``goal_dist`` (the last is optional) and, for id goals,
    ``env.goals`` as the categories (``num_categories``, default the env's ``num_goals``; 0 with coordinate goals); the default
    env is then a ``NavSyntheticEnv`` and ``info()`` carries ``spl``, ``soft_spl``, ``dist_to_goal``, ``path_length``,
    ``no_path``.  The act loop does not change.  ``env_seed``: the seed of the env the evaluator builds itself (default
    ``1000 + rank``, the ``Worker``'s).

    The agent keywords (``encoder``, ``net``, ``pooling``, ``sensors``, ``goal_ids``, ``goal_in``, ``depth``, ``zeroshot``,
    ``num_actions``, ``prev_actions``, ``prev_action_null_token``, ``rnn_type``, ``rnn_layers``, ``hidden``) are ``engine.Worker``'s:
    the same agents (documented there), the same refusals before anything is built, the same checkpoints -- one of another net,
    cell, depth or without the previous-action embedding is refused by tensor name.  An ``env=`` must serve what the agent reads:
    ``depth`` / ``goal_frames`` on the device with ``observe_second()`` (``depth=True`` / ``net="two_view"``), ``sensors``
    (``net="pooled"`` with sensors)."""

    def __init__(self, n_actors: int, T: int = 128, device="cuda:0", seed: int = 0, rank: int = 0, encoder: str = "rn50",
                 encoder_sd=None, policy_sd=None, checkpoint: Optional[str] = None, deterministic: bool = False,
                 encoder_streams: int = 2, frames_u8: bool = False, goal_in: int = 0, num_actions: int = 6,
                 zeroshot: bool = False, sync_actions: bool = False, record: bool = False, env=None, text_sd=None,
                 goal_tokens=None, encoder_chunk: int = 0, record_capacity: int = 0, nav_metrics: bool = False,
                 num_categories: Optional[int] = None, env_seed: Optional[int] = None, depth: bool = False,
                 prev_actions: int = 0, prev_action_null_token: bool = True, rnn_type: str = "GRU",
                 rnn_layers: int = 1, hidden: int = 512, net: str = "goal_encoder", pooling: str = "attnpool", sensors=(),
                 goal_ids: bool = True):
        self._configure(encoder, net, pooling, sensors, goal_ids, goal_in, depth, zeroshot, num_actions, prev_actions,
                        prev_action_null_token, rnn_type, rnn_layers, hidden, env=env)
        self._text_sd, self._goal_tokens = text_sd, goal_tokens
        assert policy_sd is None or checkpoint is None, "policy_sd and checkpoint both name the weights"
        if sync_actions not in (False, True):
            raise ValueError("Evaluator: sync_actions is False or True (one vectorised env for all actors)")
        self.nav_metrics, self._num_categories, self._env_seed = nav_metrics, num_categories, env_seed
        if nav_metrics and env is not None:
            nav_env_tensors(env, False)     # an env that cannot be scored fails here, before anything is built
        self.deterministic, self.sync_actions, self.record = deterministic, sync_actions, record
        self.dev = self.device = torch.device(device)
        if self.dev.index is None:
            self.dev = self.device = torch.device("cuda", torch.cuda.current_device())
        self.checkpoint_steps = None
        if checkpoint is not None:
            ck = torch.load(checkpoint, map_location="cpu")
            policy_sd, self.checkpoint_steps = ck["model_state_dict"], int(ck.get("total_steps", 0))
        self._checkpoint = checkpoint
        self._init(n_actors, T, seed, rank, encoder, encoder_sd, policy_sd, encoder_chunk, encoder_streams, frames_u8, env,
                   record_capacity)

    @_lib.on_device
    def _init(self, n_actors, T, seed, rank, encoder, encoder_sd, policy_sd, encoder_chunk, encoder_streams, frames_u8, env,
              record_capacity):
        self.N, self.T, self.rank = n_actors, T, rank
        N = n_actors
        d = self.dev
        if self._checkpoint is not None and self.prev_action_dims and not self.pooled_net:
            # before the handle flattens it: a checkpoint of an agent without the embedding is refused by the tensor's name
            from .synthetic import POLICY_PREV_ACTION_EMBEDDER
            if POLICY_PREV_ACTION_EMBEDDER not in policy_sd:
                raise KeyError(f"{self._checkpoint}: the checkpoint lacks the tensor {POLICY_PREV_ACTION_EMBEDDER!r} of this agent")
        encs, pools = self._build_model(n_actors, encoder, encoder_sd, policy_sd, encoder_chunk, encoder_streams)
        self.h = torch.zeros((N, self.SW), dtype=torch.float32, device=d)
        self.h_next = torch.zeros((N, self.SW), dtype=torch.float32, device=d)
        # one step's results (record=True: run() points these at the rows of the [chunks*T, ...] recordings instead)
        self._hv = torch.empty((1, N, self.A + 1), dtype=torch.float32, device=d)
        self._actions = torch.zeros((1, N), dtype=torch.int64, device=d)
        self._logp = torch.zeros((1, N), dtype=torch.float32, device=d)
        self._values = torch.zeros((1, N), dtype=torch.float32, device=d)
        self.actions = self.logp = self.values = self.hv = None
        self._prev_row = self._actions[0]       # what the next step reads as its previous actions: the last step's row (zeros at first)
        env_cls, ekw = self._env_recipe()
        env_seed = self._env_seed if self._env_seed is not None else 1000 + rank
        self.env = env if env is not None else env_cls(N, T, d, seed=env_seed, frames_u8=frames_u8, **ekw)
        assert (self.env.N, self.env.T) == (N, T), "the env's actor count and rollout length are the evaluator's"
        self.episodes = self._episode_tracker(self._num_categories, record_capacity)
        self._build_slices(n_actors, encs, pools, 2, 0, bool(self.env.host))
        self.seed = seed + 7919 * rank
        self.chunk = 0                  # chunks played so far (the sampling key's iteration; carries across run() calls)
        self.k = 0                      # env steps played so far: the feature ring's and the memory ping-pong's parity
        rgb, dep = self._observe()      # first observation
        for sl in self.slices:
            self._encode_slice(sl, rgb, 0, dep)
        torch.cuda.synchronize(d)

    # ---- one act step of a slice ----------------------------------------------------------------
    def _act_slice(self, sl, t: int, row: int):
        """Chunk step ``t`` of the slice's actors on the current stream; results go to row ``row`` of the step buffers."""
        o, n = sl.o, sl.n
        rs = slice(o, o + n)
        h_in, h_out = (self.h, self.h_next) if (self.k & 1) == 0 else (self.h_next, self.h)
        feat, feat2 = sl.feat[self.k & 1], self._f2(sl, self.k & 1)
        hv, actions, logp, values = self._hv[row][rs], self._actions[row][rs], self._logp[row][rs], self._values[row][rs]
        key = self.chunk * (self.T + 1) + t
        pa = self._prev_row[rs] if self.prev_action_dims else None
        goal = self.env.goals[t][rs] if self._has_goal else None            # (as Worker._act_slice)
        sens = self.env.sensors[t][rs] if self._has_sensors else None
        if self._act_fused:
            self.policy.act(self.params, feat, goal, h_in[rs], self.env.masks[t][rs], n, sl.ws_act, hv, h_out[rs],
                            actions, logp, values, self.seed, key, o, reuse_tables=sl.act_tables_valid,
                            deterministic=self.deterministic, feat2=feat2, prev_actions=pa, sensors=sens)
        elif self._act_wide:   # 8 to 256 actions: the wide heads launch selects (ec_policy_act_ex)
            self.policy.act_ex(self.params, feat, goal, h_in[rs], self.env.masks[t][rs], n, sl.ws_act, hv, h_out[rs],
                               actions, logp, values, self.seed, key, o, reuse_tables=sl.act_tables_valid,
                               deterministic=self.deterministic, feat2=feat2, prev_actions=pa, sensors=sens)
        else:   # the switch off: the forward, then the stand-alone selection kernel
            self.policy.forward(self.params, feat, goal, h_in[rs], self.env.masks[t][rs], 1, n, sl.ws_act,
                                hv=hv, h_final=h_out[rs], for_backward=False, reuse_tables=sl.act_tables_valid, feat2=feat2,
                                prev_actions=pa, sensors=sens)
            if self.deterministic:
                _lib.check(self.lib.ec_mode_actions(hv.data_ptr(), actions.data_ptr(), logp.data_ptr(), values.data_ptr(), n,
                                                    self.A, _lib.stream_ptr()), "ec_mode_actions")
            else:
                _lib.check(self.lib.ec_sample_actions(hv.data_ptr(), actions.data_ptr(), logp.data_ptr(), values.data_ptr(), n,
                                                      self.A, self.seed, key, o, _lib.stream_ptr()), "ec_sample_actions")
        sl.act_tables_valid = True

    @_lib.on_device
    def run(self, chunks: int = 1) -> Dict[str, float]:
        """Play ``chunks * T`` env steps; after each chunk the tracker takes the env's ``rewards`` / ``masks`` / ``success``."""
        T, N, d = self.T, self.N, self.dev
        if self.record:
            self.hv = self._hv = torch.empty((chunks * T, N, self.A + 1), dtype=torch.float32, device=d)
            self.actions = self._actions = torch.zeros((chunks * T, N), dtype=torch.int64, device=d)
            self.logp = self._logp = torch.zeros((chunks * T, N), dtype=torch.float32, device=d)
            self.values = self._values = torch.zeros((chunks * T, N), dtype=torch.float32, device=d)
        if self.sync_actions and getattr(self, "_actions_host", None) is None:
            self._actions_host = torch.empty((N,), dtype=torch.int64).pin_memory()
        for c in range(chunks):
            self._fork()
            for t in range(T):
                row = c * T + t if self.record else 0
                if self.sync_actions:
                    for sl in self.slices:
                        with self._on(sl):
                            self._act_slice(sl, t, row)
                            self._actions_host[sl.o:sl.o + sl.n].copy_(self._actions[row][sl.o:sl.o + sl.n], non_blocking=True)
                    for sl in self.slices:
                        (sl.stream if sl.stream is not None else torch.cuda.current_stream()).synchronize()
                    rgb, dep = self._observe(self._actions_host)        # env.step(actions[t])
                    for sl in self.slices:
                        with self._on(sl):
                            self._encode_slice(sl, rgb, (self.k + 1) & 1, dep)
                else:
                    rgb, dep = self._observe()    # env.step(actions[t]) happens here in the real system
                    for sl in self.slices:
                        with self._on(sl):
                            self._act_slice(sl, t, row)
                            self._encode_slice(sl, rgb, (self.k + 1) & 1, dep)
                self.k += 1
                self._prev_row = self._actions[row]
            self._join()
            self._update_episodes()
            self.chunk += 1
        return self.info()

    def info(self) -> Dict[str, float]:
        """``{"episodes", "reward", "reward_std", "ep_length", "success"}`` over the episodes completed so far (with
        ``nav_metrics`` also ``spl``, ``soft_spl``, ``dist_to_goal``, ``path_length``, ``no_path``)."""
        return self.episodes.info()


# ---- the metrics file of an evaluation run ------------------------------------------------------------------------------------
# One entry per recorded episode.  readme_files/zeroshot_objectnav.md:29-48 reads three things from the file [U] AllenAct's
# ``--eval`` writes -- ``[0]["tasks"][i]["task_info"]["object_type"]``, ``["success"]`` and ``["spl"]`` -- and only those three
# are promised in AllenAct's shape; the other keys are this project's.

def metrics_from_records(records: Dict, names: Optional[Sequence[str]] = None) -> List[Dict]:
    """``NavEpisodeTracker.records()`` -> the metrics file's content: a list holding one object whose ``"tasks"`` has one entry
    per stored episode; ``"dropped": k`` joins it when ``k`` more episodes completed than the record buffers hold.
    ``names[c]`` names goal id ``c`` (default ``str(c)``); an id without a name is written as ``str(id)``."""
    cols = {k: (v.tolist() if hasattr(v, "tolist") else list(v)) for k, v in records.items() if k != "dropped"}
    names = list(names) if names is not None else None
    tasks = []
    for i in range(len(cols["actor"])):
        c = int(cols["category"][i])
        name = names[c] if names is not None and 0 <= c < len(names) else str(c)
        tasks.append({"task_info": {"object_type": name, "actor": int(cols["actor"][i])},
                      "success": float(cols["success"][i]), "spl": float(cols["spl"][i]),
                      "soft_spl": float(cols["soft_spl"][i]), "ep_length": int(cols["length"][i]),
                      "reward": float(cols["return"][i]), "dist_to_target": float(cols["goal_dist"][i]),
                      "path_length": float(cols["path"][i])})
    top = {"tasks": tasks}
    dropped = int(records.get("dropped", 0))
    if dropped > 0:
        top["dropped"] = dropped
    return [top]


def write_metrics_json(path: str, records: Dict, names: Optional[Sequence[str]] = None) -> List[Dict]:
    metrics = metrics_from_records(records, names)
    if "dropped" in metrics[0]:
        print(f"evaluate: {metrics[0]['dropped']} episodes completed beyond the record capacity and are missing from {path}",
              file=sys.stderr)
    with open(path, "w") as f:
        json.dump(metrics, f)
    return metrics


def scores_by_object_type(metrics, names: Sequence[str]) -> Dict[str, Tuple[float, float]]:
    """``{name: (success rate, mean SPL)}`` over the episodes of each object type in a metrics file's content (the parsed JSON,
    or its path); a type without episodes scores ``(nan, nan)``."""
    if isinstance(metrics, str):
        with open(metrics) as f:
            metrics = json.load(f)
    sums = {name: [0, 0.0, 0.0] for name in names}
    for task in metrics[0]["tasks"]:
        s = sums.get(task["task_info"]["object_type"])
        if s is not None:
            s[0] += 1
            s[1] += task["success"]
            s[2] += task["spl"]
    nan = float("nan")
    return {name: (s[1] / s[0], s[2] / s[0]) if s[0] else (nan, nan) for name, s in sums.items()}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m embodied_clip_amd.evaluate",
                                 description="Run an agent for chunks x steps env steps on the synthetic env and print its episode metrics.")
    ap.add_argument("--checkpoint", default=None, help="a file written by Worker.save_checkpoint (policy weights; the encoder stays the seeded stand-in)")
    ap.add_argument("--encoder", default="rn50")
    ap.add_argument("--actors", type=int, default=64)
    ap.add_argument("--steps", type=int, default=128, help="env steps per chunk (the rollout length T)")
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--deterministic", action="store_true", help="CategoricalDistr.mode() instead of sample()")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--goal-in", type=int, default=0)
    ap.add_argument("--num-actions", type=int, default=6)
    ap.add_argument("--zeroshot", action="store_true")
    ap.add_argument("--frames-u8", action="store_true")
    ap.add_argument("--depth", action="store_true", help="the RGB-D agent: a depth tower beside the RGB tower, dual goal encoder (encoder rn50 / rn50x16); with --net pooled "
                    "--pooling avgpool: the Habitat RGB-D encoder, both towers' maps summed and average-pooled")
    ap.add_argument("--sync-actions", action="store_true")
    ap.add_argument("--prev-actions", type=int, default=0, metavar="E",
                    help="the agent conditions on its previous action through an E-wide embedding (0: off; AllenAct's default is 6, Habitat's 32)")
    ap.add_argument("--no-prev-action-null-token", action="store_true",
                    help="with --prev-actions: no null row for an episode's first step (action a is row a)")
    ap.add_argument("--rnn-type", default="GRU", choices=("GRU", "LSTM"), help="the recurrent cell of the agent (and of its checkpoint)")
    ap.add_argument("--rnn-layers", type=int, default=1, choices=(1, 2, 3, 4), help="recurrent layers of the agent (and of its checkpoint)")
    ap.add_argument("--net", default="goal_encoder", choices=("goal_encoder", "pooled", "two_view"),
                    help="pooled: the Habitat DD-PPO net over the pooled embedding (PolicyHandle.pooled); two_view: the rearrangement agent over the "
                         "current and the goal-state view (PolicyHandle.two_view)")
    ap.add_argument("--pooling", default="attnpool", choices=("attnpool", "avgpool", "cls"),
                    help="with --net pooled: how the tower is pooled ('cls': the class embedding of --encoder vit)")
    ap.add_argument("--sensors", default="", metavar="K1,K2", help="with --net pooled: the widths of the env's float sensors, e.g. 2,2 (GPS, compass) or 3")
    ap.add_argument("--no-goal-ids", action="store_true", help="with --net pooled: no goal-id embedding (PointNav: --sensors 3)")
    ap.add_argument("--json", default=None, metavar="OUT", help="also write the info dict to this file")
    ap.add_argument("--env-seed", type=int, default=None, help="seed of the synthetic env (default 1000, what Evaluator builds itself)")
    ap.add_argument("--nav-metrics", action="store_true", help="also SPL, SoftSPL, distance to goal, and the scores per object type")
    ap.add_argument("--object-types", default=None, metavar="FILE", help="a JSON list of names, one per goal id (default \"0\", \"1\", ...)")
    ap.add_argument("--groups", default=None, metavar="FILE", help="a JSON object {group: [names]}: the scores over each group's episodes")
    ap.add_argument("--metrics-json", default=None, metavar="OUT", help="one entry per episode, in the shape the per-object-type readers expect")
    a = ap.parse_args(argv)
    if (a.object_types or a.groups or a.metrics_json) and not a.nav_metrics:
        ap.error("--object-types, --groups and --metrics-json go with --nav-metrics")
    if (a.object_types or a.groups) and a.goal_in:
        ap.error("--object-types and --groups name goal ids; --goal-in > 0 gives coordinate goals, which have no categories")
    names = groups = None
    if a.object_types:
        with open(a.object_types) as f:
            names = json.load(f)
        if isinstance(names, dict):         # (the fixture's shape: {"object_types": [...], ...})
            names = names["object_types"]
    if a.groups:
        with open(a.groups) as f:
            groups = json.load(f)
        groups = {k: v for k, v in groups.items() if k != "object_types"}
    print("evaluate: the frozen encoder holds the seeded stand-in weights (a checkpoint carries the policy only)", file=sys.stderr)
    if a.checkpoint is None:
        print("evaluate: no --checkpoint given: using the seeded stand-in weights (an untrained agent)", file=sys.stderr)
    ev = Evaluator(a.actors, T=a.steps, seed=a.seed, env_seed=a.env_seed, encoder=a.encoder, checkpoint=a.checkpoint, deterministic=a.deterministic,
                   goal_in=a.goal_in, num_actions=a.num_actions, zeroshot=a.zeroshot, frames_u8=a.frames_u8,
                   sync_actions=a.sync_actions, nav_metrics=a.nav_metrics, depth=a.depth, prev_actions=a.prev_actions,
                   prev_action_null_token=not a.no_prev_action_null_token, rnn_type=a.rnn_type, rnn_layers=a.rnn_layers,
                   net=a.net, pooling=a.pooling, sensors=tuple(int(k) for k in a.sensors.split(",") if k), goal_ids=not a.no_goal_ids,
                   num_categories=len(names) if (names is not None and not a.goal_in) else None,
                   # every actor can end an episode at every step: the metrics file then misses none
                   record_capacity=a.chunks * a.steps * a.actors if a.metrics_json else 0)
    info = ev.run(a.chunks)
    torch.cuda.synchronize()
    if a.nav_metrics:
        tr = ev.episodes
        names = category_names(tr.C, names) if tr.C else []
        info = dict(info, by_object_type=tr.info_by_category(names) if tr.C else {},
                    groups=tr.info_groups(groups, names) if (groups and tr.C) else {})
        if a.metrics_json:
            if not tr.C:
                print("evaluate: coordinate goals have no object types: every task's object_type is written as \"-1\"", file=sys.stderr)
            write_metrics_json(a.metrics_json, tr.records(), names)
    info = dict(info, env_steps=a.chunks * a.steps * a.actors, deterministic=bool(a.deterministic),
                policy_weights=a.checkpoint or "seeded stand-in", encoder_weights="seeded stand-in", checkpoint_steps=ev.checkpoint_steps)
    print(json.dumps(info))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(info, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
