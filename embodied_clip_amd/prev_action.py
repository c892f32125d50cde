"""Previous-action embedding of the recurrent input: the HIP kernels of csrc/prev_action.hip, each alone.

Mirrors [U] habitat_baselines ``PointNavResNetPolicy`` (``prev_action_embedding = nn.Embedding(num_actions + 1, 32)`` indexed by
``((prev_actions.float() + 1) * masks).long()``) and [U] allenact ``VisualNavActorCritic`` (``add_prev_actions``,
``action_embed_size``, ``add_prev_action_null_token``).  Both are restated from the published sources, which are not under the
reference tree: parity is unpinned.

The embedding ``Emb [R, E]`` (``R = num_actions + null``) is concatenated to the GRU input, so it reaches the network through
``gi = x' . weight_ih^T`` alone.  With ``Wa = weight_ih[:, flat:flat + E]`` the three functions here are

    PT  = Emb . Wa^T                       ``prev_action_table``   (weight-derived, like the goal table E1)
    gi[b] += PT[idx[b]]                    ``prev_action_add_``
    dEmb += dPT . Wa,  dWa += dPT^T . Emb  ``prev_action_grad_``   (dPT[r] = the ordered sum of dgi[b] over idx[b] == r)

and nothing ``[T*N, E]``-shaped exists.  ``idx`` is formed inside the kernels from ``prev_actions`` (int64), ``masks`` and the
null flag; an index outside ``[0, R)`` is never dereferenced.  ``weight_ih`` is passed whole with the column offset: its row
stride ``flat + E`` need not be a multiple of 4.  ``PolicyHandle(prev_action_dims=E)`` runs the same launches inside the
policy (``ec_policy_forward_pa`` / ``ec_policy_act_pa``); these wrappers are the kernels alone.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib


def _check(t: torch.Tensor, dtype, what: str) -> None:
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), f"{what}: a contiguous {dtype} tensor on the GPU is needed"


def _weight(w: torch.Tensor, col0: int, E: int):
    _check(w, torch.float32, "weight")
    assert w.dim() == 2 and 0 <= col0 and col0 + E <= w.shape[1], f"columns {col0}..{col0 + E} lie outside weight {tuple(w.shape)}"
    return w.shape[0], w.shape[1]


def prev_action_table(emb: torch.Tensor, w: torch.Tensor, col0: int, null_token: bool, out: Optional[torch.Tensor] = None):
    """``PT [R, G] = emb . w[:, col0:col0 + E]^T`` (fp32 FMA in ascending ``e``).  emb ``[R, E]``, w ``[G, ld]``."""
    _check(emb, torch.float32, "emb")
    R, E = emb.shape
    G, ld = _weight(w, col0, E)
    if out is None:
        out = torch.empty(R, G, dtype=torch.float32, device=emb.device)
    _check(out, torch.float32, "out")
    assert out.shape == (R, G)
    with _lib.tensor_guard(emb):
        _lib.check(_lib.load().ec_prev_action_table(emb.data_ptr(), w.data_ptr(), ld, col0, out.data_ptr(), R - int(null_token),
                                                    int(null_token), G, E, _lib.stream_ptr()), "ec_prev_action_table")
    return out


def prev_action_add_(gi: torch.Tensor, pt: torch.Tensor, prev_actions: torch.Tensor, masks: Optional[torch.Tensor],
                     null_token: bool):
    """``gi[b] += pt[idx[b]]`` in place.  gi ``[B, G]``, pt ``[R, G]``, prev_actions int64 ``[B]``, masks fp32 ``[B]`` (may be
    None without the null token)."""
    _check(gi, torch.float32, "gi")
    _check(pt, torch.float32, "pt")
    _check(prev_actions, torch.int64, "prev_actions")
    B, G = gi.shape
    assert pt.shape[1] == G and prev_actions.numel() == B
    assert not null_token or masks is not None, "the null token is selected by masks"
    if masks is not None:
        _check(masks, torch.float32, "masks")
        assert masks.numel() == B
    with _lib.tensor_guard(gi):
        _lib.check(_lib.load().ec_prev_action_add(gi.data_ptr(), pt.data_ptr(), prev_actions.data_ptr(), _lib.ptr(masks),
                                                  int(null_token), pt.shape[0] - int(null_token), B, G, _lib.stream_ptr()),
                   "ec_prev_action_add")
    return gi


def prev_action_grad_scratch(B: int, G: int, num_actions: int, null_token: bool, device) -> torch.Tensor:
    """The scratch of ``prev_action_grad_`` (owned by one stream at a time); its first ``R * G`` floats hold ``dPT`` afterwards."""
    n = _lib.load().ec_prev_action_grad_scratch_floats(B, G, num_actions, int(null_token))
    assert n > 0, (B, G, num_actions, null_token)
    return torch.empty(n, dtype=torch.float32, device=device)


def prev_action_grad_(dgi: torch.Tensor, prev_actions: torch.Tensor, masks: Optional[torch.Tensor], null_token: bool,
                      emb: torch.Tensor, w: torch.Tensor, col0: int, demb: torch.Tensor, dw: torch.Tensor,
                      scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adds the embedding's gradient onto ``demb [R, E]`` and ``weight_ih``'s onto columns ``col0..col0 + E`` of ``dw`` (shaped
    like ``w``); returns ``dPT [R, G]``, a view of the scratch.  Deterministic: two calls give the same bits."""
    _check(dgi, torch.float32, "dgi")
    _check(prev_actions, torch.int64, "prev_actions")
    _check(emb, torch.float32, "emb")
    _check(demb, torch.float32, "demb")
    _check(dw, torch.float32, "dw")
    B, G = dgi.shape
    R, E = emb.shape
    Gw, ld = _weight(w, col0, E)
    assert Gw == G and dw.shape == w.shape and demb.shape == emb.shape and prev_actions.numel() == B
    assert not null_token or masks is not None, "the null token is selected by masks"
    if masks is not None:
        _check(masks, torch.float32, "masks")
        assert masks.numel() == B
    A = R - int(null_token)
    if scratch is None:
        scratch = prev_action_grad_scratch(B, G, A, null_token, dgi.device)
    _check(scratch, torch.float32, "scratch")
    lib = _lib.load()
    assert scratch.numel() >= lib.ec_prev_action_grad_scratch_floats(B, G, A, int(null_token))
    with _lib.tensor_guard(dgi):
        _lib.check(lib.ec_prev_action_grad(dgi.data_ptr(), prev_actions.data_ptr(), _lib.ptr(masks), int(null_token), A,
                                           emb.data_ptr(), w.data_ptr(), ld, col0, demb.data_ptr(), dw.data_ptr(),
                                           scratch.data_ptr(), B, G, E, _lib.stream_ptr()), "ec_prev_action_grad")
    return scratch[:R * G].view(R, G)
