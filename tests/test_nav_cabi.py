"""``ec_nav_episode_stats`` on a box without a GPU: exported, bound, and its argument checks come before any HIP call."""
import ctypes


def test_symbol_is_exported_and_bound():
    from embodied_clip_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "ec_nav_episode_stats")
    res, args = _lib.SIGNATURES["ec_nav_episode_stats"]
    assert res is ctypes.c_int and len(args) == 19
    # ec_episode_stats with four inputs + C behind `success` and one more carry
    old = _lib.SIGNATURES["ec_episode_stats"][1]
    assert args == old[:3] + [ctypes.c_void_p] * 4 + [ctypes.c_int] + old[3:5] + [ctypes.c_void_p] + old[5:]


def _call(lib, rewards=1, masks=1, success=None, step_dist=1, start_dist=1, goal_dist=None, category=None, C=0, carry_ret=1,
          carry_len=1, carry_path=1, totals=1, rec_f=None, rec_i=None, cap=0, n_records=1, T=4, N=5):
    return lib.ec_nav_episode_stats(rewards, masks, success, step_dist, start_dist, goal_dist, category, C, carry_ret, carry_len,
                                    carry_path, totals, rec_f, rec_i, cap, n_records, T, N, None)


def test_argument_checks_come_first():
    from embodied_clip_amd import _lib
    lib = _lib.load()
    ARG, SHAPE = -1, -2
    for required in ("rewards", "masks", "step_dist", "start_dist", "carry_ret", "carry_len", "carry_path", "totals", "n_records"):
        assert _call(lib, **{required: None}) == ARG, required
    assert _call(lib, rec_f=1, cap=8) == ARG                        # one record buffer without the other
    assert _call(lib, rec_i=1, cap=8) == ARG
    assert _call(lib, category=1, C=0) == ARG                       # ids without rows to count them in
    assert _call(lib, category=None, C=3) == ARG                    # rows without ids
    assert _call(lib, T=0) == SHAPE
    assert _call(lib, N=0) == SHAPE
    assert _call(lib, cap=-1) == SHAPE
    assert _call(lib, category=1, C=-1) == SHAPE
    assert _call(lib, category=1, C=65) == SHAPE
    assert b"shape" in lib.ec_strerror(SHAPE)
