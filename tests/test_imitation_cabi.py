"""Argument validation of the imitation entry points: it happens before any HIP call, so it runs without a GPU."""
EC_ERR_ARG, EC_ERR_SHAPE = -1, -2
P = 4096        # a non-NULL stand-in pointer: never dereferenced, every call below is refused first


def _lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def test_scratch_size():
    assert _lib().ec_imitation_scratch_doubles() > 0


def test_imitation_loss_refuses_bad_arguments():
    lib = _lib()
    ok = [P, P, P, None, P, P, P, 4, 6, 1.0, 1.0, 0, None]          # (denom may be NULL)
    for i in (0, 1, 2, 4, 5, 6):
        a = list(ok)
        a[i] = None
        assert lib.ec_imitation_loss(*a) == EC_ERR_ARG, i
    for B in (0, -3):
        a = list(ok)
        a[7] = B
        assert lib.ec_imitation_loss(*a) == EC_ERR_SHAPE, B
    for A in (0, 257, -1):
        a = list(ok)
        a[8] = A
        assert lib.ec_imitation_loss(*a) == EC_ERR_SHAPE, A


def test_expert_count_refuses_bad_arguments():
    lib = _lib()
    assert lib.ec_expert_count(None, 3, 4, 0, 4, P, None) == EC_ERR_ARG
    assert lib.ec_expert_count(P, 3, 4, 0, 4, None, None) == EC_ERR_ARG
    for T, N, n0, n1 in ((0, 4, 0, 4), (3, 0, 0, 1), (3, 4, -1, 2), (3, 4, 2, 2), (3, 4, 3, 2), (3, 4, 0, 5)):
        assert lib.ec_expert_count(P, T, N, n0, n1, P, None) == EC_ERR_SHAPE, (T, N, n0, n1)


def test_teacher_force_refuses_bad_arguments():
    lib = _lib()
    ok = [P, P, P, 0.5, P, P, 4, 6, 1, 0, 0, None]
    for i in (0, 1, 2, 4, 5):
        a = list(ok)
        a[i] = None
        assert lib.ec_teacher_force(*a) == EC_ERR_ARG, i
    for p in (-0.1, 1.1, float("nan")):
        a = list(ok)
        a[3] = p
        assert lib.ec_teacher_force(*a) == EC_ERR_ARG, p
    for N, A in ((0, 6), (-1, 6), (4, 0)):
        a = list(ok)
        a[6], a[7] = N, A
        assert lib.ec_teacher_force(*a) == EC_ERR_SHAPE, (N, A)


def test_python_surface():
    import inspect
    from embodied_clip_amd import imitation as il
    from embodied_clip_amd.engine import SyntheticEnv, Worker
    kw = inspect.signature(Worker.__init__).parameters
    assert kw["loss"].default == "ppo" and kw["il_weight"].default == 1.0 and kw["teacher_forcing"].default is None
    assert inspect.signature(SyntheticEnv.__init__).parameters["expert"].default is False
    assert issubclass(il.Imitation, il.AbstractActorCriticLoss)
