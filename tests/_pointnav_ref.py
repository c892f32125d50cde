"""CPU reference of the PointNav actor-critic for the PointNav tests (test infrastructure only).

A torch restatement of [U] allenai/allenact ~v0.5.0 ``projects/pointnav_baselines/models/point_nav_models.py``
``ResnetTensorPointNavActorCritic``: the ObjectNav model of ``oracle/policy.py`` with ``embed_class = nn.Embedding(n, 32)``
replaced by ``embed_goal = nn.Linear(goal_in, 32)`` on the goal sensor's float vector (polar ``(rho, phi)``); the embedding
is viewed ``[B, 32, 1, 1]``, expanded over the feature grid and concatenated AFTER the compressed features.  Not under the
reference tree: restated from the published source, parity unpinned.  The recurrence and the heads are the oracle's own
(imported, not copied); ``as_oracle_policy()`` puts this forward in ``oracle.policy.actor_critic_forward``'s place for the
duration of a ``with`` block, so that ``oracle.ppo.ppo_update_step`` serves unchanged (its ``batch["goal"]`` is then the
float ``[T, N, goal_in]`` goal).
"""
import contextlib
from typing import Dict
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import policy as opol

P = "goal_visual_encoder."


def goal_encoder(feat: torch.Tensor, goal_vec: torch.Tensor, sd: Dict[str, torch.Tensor]) -> torch.Tensor:
    """feat: [B, C, H, W]; goal_vec: [B, goal_in] float -> [B, 32*H*W] (channel-major flatten)."""
    x = F.relu(F.conv2d(feat, sd[P + "resnet_compressor.0.weight"], sd[P + "resnet_compressor.0.bias"]))
    x = F.relu(F.conv2d(x, sd[P + "resnet_compressor.2.weight"], sd[P + "resnet_compressor.2.bias"]))
    emb = F.linear(goal_vec, sd[P + "embed_goal.weight"], sd[P + "embed_goal.bias"])          # [B, 32]
    emb = emb.view(emb.shape[0], emb.shape[1], 1, 1).expand(-1, -1, x.shape[-2], x.shape[-1])
    x = torch.cat([x, emb], dim=1)
    x = F.relu(F.conv2d(x, sd[P + "target_obs_combiner.0.weight"], sd[P + "target_obs_combiner.0.bias"]))
    x = F.conv2d(x, sd[P + "target_obs_combiner.2.weight"], sd[P + "target_obs_combiner.2.bias"])
    return x.reshape(x.shape[0], -1)


def actor_critic_forward(feat, goal_vec, h0, masks, sd):
    """feat: [T, N, C, H, W]; goal_vec: [T, N, goal_in]; h0: [1, N, hidden]; masks: [T, N, 1]
    -> (logits [T, N, A], values [T, N, 1], h [1, N, hidden])."""
    T, N = feat.shape[:2]
    x = goal_encoder(feat.reshape(T * N, *feat.shape[2:]), goal_vec.reshape(T * N, -1), sd).view(T, N, -1)
    out, h = opol.rnn_state_encoder(x, h0, masks, sd)
    logits = F.linear(out, sd["actor.linear.weight"], sd["actor.linear.bias"])
    values = F.linear(out, sd["critic.fc.weight"], sd["critic.fc.bias"])
    return logits, values, h


@contextlib.contextmanager
def as_oracle_policy():
    with mock.patch.object(opol, "actor_critic_forward", actor_critic_forward):
        yield
