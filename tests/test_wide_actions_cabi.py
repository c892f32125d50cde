"""The entry points of the wide action space on a box without a GPU: exported, bound, and every argument check in front of the
first HIP call; the narrow entry points keep their limits."""
import ctypes as C

import pytest

NEW = ("ec_heads_wide", "ec_policy_act_ex", "ec_ppo_loss_wide", "ec_ppo_loss_wide_scratch_doubles")
P = 64        # a non-NULL "pointer": the checks under test return before anything is read


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def _policy(lib, num_actions, **kw):
    from embodied_clip_amd import _lib
    cfg = dict(in_channels=128, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=num_actions, compress_hid=128,
               compress_out=32, comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0)
    cfg.update(kw)
    h = C.c_void_p()
    assert lib.ec_policy_create(C.byref(h), C.byref(_lib.PolicyCfg(**cfg))) == 0
    return h


def test_symbols_are_exported_and_bound(lib):
    from embodied_clip_amd import _lib
    for n in NEW:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.ec_ppo_loss_wide_scratch_doubles() == 4 * 1024 + 1


def test_ppo_loss_wide_argument_checks(lib):
    ok = [P] * 9
    for i in range(9):
        a = list(ok)
        a[i] = None
        assert lib.ec_ppo_loss_wide(*a, 8, 84, 0.1, 0.1, 0.5, 0.01, 1.0, None) == -1, i
    for A in (0, 257, -3):
        assert lib.ec_ppo_loss_wide(*ok, 8, A, 0.1, 0.1, 0.5, 0.01, 1.0, None) == -2, A
    assert lib.ec_ppo_loss_wide(*ok, 0, 84, 0.1, 0.1, 0.5, 0.01, 1.0, None) == -2


def test_ppo_loss_ex_keeps_its_bound(lib):
    assert lib.ec_ppo_loss_ex(*([P] * 8), 8, 17, 0.1, 0.1, 0.5, 0.01, 1.0, None) == -2
    assert lib.ec_ppo_loss_ex(*([P] * 8), 8, 0, 0.1, 0.1, 0.5, 0.01, 1.0, None) == -2


def test_heads_wide_argument_checks(lib):
    def call(hs=P, Wa=P, ba=P, wc=P, bc=P, hv=P, B=5, H=512, A=84, actions=P, logp=P, values=P, greedy=0, first=0, ea=None, em=None,
             p=0.0):
        return lib.ec_heads_wide(hs, Wa, ba, wc, bc, hv, B, H, A, actions, logp, values, greedy, 1, 2, first, ea, em, p, None)
    for k in ("hs", "Wa", "ba", "wc", "bc", "hv"):
        assert call(**{k: None}) == -1, k
    assert call(logp=None) == -1
    for A in (0, 257):
        assert call(A=A) == -2, A
    assert call(B=0) == -2 and call(H=510) == -2 and call(H=0) == -2 and call(first=-1) == -2
    assert call(ea=P, em=P, p=0.5, greedy=1) == -1                # forcing with greedy
    assert call(ea=P, em=None, p=0.5) == -1 and call(ea=None, em=P, p=0.5) == -1
    assert call(ea=P, em=P, p=1.5) == -1 and call(ea=P, em=P, p=float("nan")) == -1 and call(p=0.5) == -1
    assert call(ea=P, em=P, p=0.5, actions=None, logp=None) == -1


def test_policy_act_ex_argument_checks(lib):
    h = _policy(lib, 84)
    try:
        def call(handle=h, actions=P, logp=P, greedy=0, ea=None, em=None, p=0.0, first=0, goal=P, goal_vec=None, params=P):
            return lib.ec_policy_act_ex(handle, params, P, None, 1, goal, goal_vec, P, P, 4, P, 1 << 30, 0, P, P, actions, logp, P, greedy,
                                        1, 2, first, ea, em, p, None)
        assert call(handle=None) == -1 and call(actions=None) == -1 and call(logp=None) == -1
        assert call(ea=P, em=P, p=0.5, greedy=1) == -1            # forcing with greedy
        assert call(ea=P, em=None, p=0.5) == -1 and call(p=0.25) == -1 and call(ea=P, em=P, p=-0.1) == -1
        assert call(first=-1) == -2
        assert call(params=None) == -1
        assert call(goal=None) == -1 and call(goal=P, goal_vec=P) == -1          # the goal argument of the handle's type, alone
    finally:
        lib.ec_policy_destroy(h)
    h = _policy(lib, 257)
    try:
        assert lib.ec_policy_act_ex(h, P, P, None, 1, P, None, P, P, 4, P, 1 << 30, 0, P, P, P, P, P, 0, 1, 2, 0, None, None, 0.0, None) == -6
    finally:
        lib.ec_policy_destroy(h)


def test_narrow_act_entry_points_still_refuse_nine_actions(lib):
    h = _policy(lib, 9)
    try:
        assert lib.ec_policy_act_greedy(h, P, P, None, 1, P, P, P, 4, P, 1 << 30, 0, P, P, P, P, P, None) == -6
        assert lib.ec_policy_act(h, P, P, None, 1, P, P, P, 4, P, 1 << 30, 0, P, P, P, P, P, 1, 2, 0, None) == -6
    finally:
        lib.ec_policy_destroy(h)
