"""Imitation learning over the HIP kernels: the expert cross-entropy loss, teacher forcing and its schedules.

Mirrors [U] allenai/allenact ~v0.5.0 (the training method of readme_files/baselines_ithor_rearrangement.md -- DAgger --
and of AllenAct's behaviour-cloning / DAgger configurations of the ObjectNav and PointNav agents; restated, parity unpinned):

  * ``Imitation`` == ``allenact/algorithms/onpolicy_sync/losses/imitation.py`` ``Imitation`` for a ``CategoricalDistr``
    and an ``expert_action`` observation ``[..., 2]`` = (action, mask):
    ``-(mask * log_prob(action)).sum() / mask.sum().clamp(min=1)``;
  * ``teacher_force`` == ``TeacherForcingDistr.sample`` / ``log_prob`` (``base_abstractions/distributions.py``) as one small
    launch behind the act step;
  * ``LinearDecay`` / ``StepwiseLinearDecay`` == the schedules of ``allenact/utils/experiment_utils.py`` that experiment
    configs pass as ``teacher_forcing=``, plain callables of the step count.

The rearrangement agent's two-view MODEL is not built (README.md): the loss runs on the agents there are.
"""
from __future__ import annotations

from bisect import bisect_right
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .allenact_compat import AbstractActorCriticLoss


def imitation_scratch(device) -> torch.Tensor:
    """The loss kernel's partial-sum scratch (one per stream that calls it)."""
    return torch.zeros(_lib.load().ec_imitation_scratch_doubles(), dtype=torch.float64, device=device)


def imitation_loss_raw(hv, expert_actions, expert_mask, A: int, weight: float = 1.0, grad_scale: float = 1.0,
                       denom: Optional[torch.Tensor] = None, dhv: Optional[torch.Tensor] = None,
                       sums: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, accumulate: bool = False):
    """Fused loss forward+backward.  hv [B, A+1] fp32 contiguous; expert_actions int64 [B]; expert_mask fp32 [B].
    ``denom``: a float64 device scalar that replaces this call's own ``mask.sum()`` (the calls that split one minibatch share
    it).  ``accumulate``: add the gradient term to ``dhv`` (which then must be given) instead of writing it.
    Returns (dhv [B, A+1], sums3 float64 device tensor = {sum mask * -logp_expert, sum mask, sum mask * [argmax == expert]}).
    An expert id outside [0, A) on a row with mask != 0 makes sums3[0] (and so the loss) NaN."""
    lib = _lib.load()
    B = hv.shape[0]
    if accumulate and dhv is None:
        raise ValueError("imitation_loss_raw(accumulate=True) adds to a given dhv")
    if dhv is None:
        dhv = torch.empty_like(hv)
    if sums is None:
        sums = torch.empty(3, dtype=torch.float64, device=hv.device)
    if scratch is None:
        scratch = imitation_scratch(hv.device)
    with _lib.tensor_guard(hv):
        _lib.check(lib.ec_imitation_loss(hv.data_ptr(), expert_actions.data_ptr(), expert_mask.data_ptr(), _lib.ptr(denom),
                                         dhv.data_ptr(), sums.data_ptr(), scratch.data_ptr(), B, A, weight, grad_scale,
                                         1 if accumulate else 0, _lib.stream_ptr()), "ec_imitation_loss")
    return dhv, sums


def expert_count(expert_mask: torch.Tensor, n0: int, n1: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``expert_mask[:, n0:n1].sum()`` of a contiguous fp32 [T, N] mask as a float64 device scalar, in a fixed order."""
    T, N = expert_mask.shape
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=expert_mask.device)
    with _lib.tensor_guard(expert_mask):
        _lib.check(_lib.load().ec_expert_count(expert_mask.data_ptr(), T, N, n0, n1, out.data_ptr(), _lib.stream_ptr()),
                   "ec_expert_count")
    return out


def teacher_force(hv, expert_actions, expert_mask, p: float, actions, logp, A: int, seed: int, step: int, first_actor: int = 0):
    """In place: where ``expert_mask != 0`` and the row's uniform (keyed by seed, step, first_actor + row) is below ``p``,
    ``actions`` becomes the expert's and ``logp`` its log-probability under ``hv[:, :A]``; other rows are untouched."""
    N = hv.shape[0]
    with _lib.tensor_guard(hv):
        _lib.check(_lib.load().ec_teacher_force(hv.data_ptr(), expert_actions.data_ptr(), expert_mask.data_ptr(), p,
                                                actions.data_ptr(), logp.data_ptr(), N, A, seed, step, first_actor,
                                                _lib.stream_ptr()), "ec_teacher_force")


class _ImitationLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hv, expert_actions, expert_mask, A):
        # (the normaliser from one small launch: without it every block of the loss kernel sums the whole mask itself)
        denom = expert_count(expert_mask.view(1, -1), 0, expert_mask.numel())
        dhv, sums = imitation_loss_raw(hv, expert_actions, expert_mask, A, denom=denom)
        total = (sums[0] / sums[1].clamp(min=1.0)).to(torch.float32)
        ctx.save_for_backward(dhv)
        ctx.mark_non_differentiable(sums)
        return total, sums

    @staticmethod
    def backward(ctx, gtotal, _gs):
        (dhv,) = ctx.saved_tensors
        return dhv * gtotal, None, None, None


class Imitation(AbstractActorCriticLoss):
    """Drop-in for AllenAct's ``Imitation`` loss (an ``AbstractActorCriticLoss``; the real ABC when allenact is importable):
    expert cross-entropy on ``batch["observations"]["expert_action"]`` ``[T, N, 2]`` = (action, mask).  Expert DISTRIBUTIONS
    (``expert_policy``) and grouped expert sensors are not implemented."""

    def __init__(self, expert_sensor=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if expert_sensor is not None and getattr(expert_sensor, "use_groups", False):
            raise NotImplementedError("Imitation: grouped expert sensors (use_groups) are not implemented")
        self.expert_sensor = expert_sensor

    def loss(self, step_count: int, batch: Dict[str, torch.Tensor], actor_critic_output, *args,
             **kwargs) -> Tuple[torch.Tensor, Dict[str, float]]:
        observations = batch["observations"]
        if "expert_action" not in observations:
            if "expert_policy" in observations:
                raise NotImplementedError("Imitation: `expert_policy` (distribution) targets are not implemented; "
                                          "only `expert_action` is")
            raise NotImplementedError("Imitation loss requires either `expert_action` or `expert_policy` sensor to be active")
        ea = observations["expert_action"]
        assert ea.shape[-1] == 2, "expert_action is (action, mask) in its last dimension"
        logits = actor_critic_output.distributions.logits
        A = logits.shape[-1]
        B = logits.numel() // A
        assert ea.numel() == 2 * B, (tuple(ea.shape), tuple(logits.shape))
        ea = ea.reshape(B, 2)
        # (the value column of hv takes no gradient from this loss)
        hv = torch.cat([logits.reshape(B, A).to(torch.float32), logits.new_zeros((B, 1), dtype=torch.float32)], dim=1).contiguous()
        total, sums = _ImitationLossFn.apply(hv, ea[:, 0].to(torch.int64).contiguous(), ea[:, 1].to(torch.float32).contiguous(), A)
        return total, {"expert_cross_entropy": float(total.detach())}


class LinearDecay:
    """``LinearDecay(steps, startp, endp)``: ``startp`` at step 0, linear to ``endp`` at ``steps``, constant after."""

    def __init__(self, steps: int, startp: float = 1.0, endp: float = 0.0):
        self.steps, self.startp, self.endp = steps, startp, endp

    def __call__(self, epoch: int) -> float:
        epoch = max(min(epoch, self.steps), 0)
        return self.startp + (self.endp - self.startp) * (epoch / float(self.steps))


class StepwiseLinearDecay:
    """``StepwiseLinearDecay([(cumulative steps, value), ...])``: piecewise linear between the given points, the first value
    before the first point and the last value from the last point on."""

    def __init__(self, cumm_steps_and_values: Sequence[Tuple[int, float]]):
        assert len(cumm_steps_and_values) >= 1
        self.steps_and_values = sorted(cumm_steps_and_values)
        self.steps = [s for s, _ in self.steps_and_values]

    def __call__(self, epoch: int) -> float:
        epoch = max(epoch, 0)
        i = bisect_right(self.steps, epoch)
        if i == 0:
            return float(self.steps_and_values[0][1])
        if i == len(self.steps):
            return float(self.steps_and_values[-1][1])
        (s0, v0), (s1, v1) = self.steps_and_values[i - 1], self.steps_and_values[i]
        return v0 + (v1 - v0) * ((epoch - s0) / float(s1 - s0))
