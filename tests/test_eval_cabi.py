"""The evaluation entry points on a box without a GPU: exported, bound, and their argument checks come before any HIP call."""
import ctypes


NEW = ("ec_policy_act_greedy", "ec_policy_act_vec_greedy", "ec_mode_actions", "ec_episode_stats")


def test_new_symbols_are_exported_and_bound():
    from embodied_clip_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    # the greedy act entry points are the sampling ones without seed, step, first_actor
    for g, s in (("ec_policy_act_greedy", "ec_policy_act"), ("ec_policy_act_vec_greedy", "ec_policy_act_vec")):
        ga, sa = _lib.SIGNATURES[g][1], _lib.SIGNATURES[s][1]
        assert ga == sa[:-4] + sa[-1:], (g, s)


def test_argument_checks_come_first():
    from embodied_clip_amd import _lib
    lib = _lib.load()
    assert lib.ec_episode_stats(None, None, None, None, None, None, None, None, 0, None, 4, 5, None) == -1
    assert lib.ec_episode_stats(1, 1, None, 1, 1, 1, 1, None, 8, 1, 4, 5, None) == -1     # one record buffer without the other
    assert lib.ec_episode_stats(1, 1, None, 1, 1, 1, None, None, 0, 1, 0, 5, None) == -2  # T = 0
    assert lib.ec_episode_stats(1, 1, None, 1, 1, 1, None, None, -1, 1, 4, 5, None) == -2  # negative capacity
    assert lib.ec_mode_actions(None, None, None, None, 4, 6, None) == -1
    assert lib.ec_mode_actions(1, 1, 1, None, 0, 6, None) == -2
    # NULL actions -> EC_ERR_ARG, whatever else is passed
    assert lib.ec_policy_act_greedy(None, None, None, None, 1, None, None, None, 4, None, 0, 0, None, None, None, None, None, None) == -1
    assert lib.ec_policy_act_vec_greedy(None, None, None, None, 1, None, None, None, 4, None, 0, 0, None, None, None, None, None, None) == -1
    # ... and more than 7 actions -> EC_ERR_UNSUPPORTED before anything is launched
    from embodied_clip_amd.policy import PolicyHandle
    h = PolicyHandle(num_actions=9)
    assert lib.ec_policy_act_greedy(h.h, 1, 1, None, 1, 1, 1, 1, 4, 1, 0, 0, 1, 1, 1, 1, None, None) == -6
