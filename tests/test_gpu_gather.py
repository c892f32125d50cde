"""The learn pass's batch gather (``Worker.gather``): every column it returns is the rollout storage's own rows, bit for bit.

Eight actors in two slices of four, three minibatch ranges ([0, 3), [3, 5), [5, 8)): every part ``update()`` forms is a PARTIAL
range of its slice (a copy, the features through the staging buffers), on both sides of the slice boundary at actor 4.  The
whole slice (used in place) is checked as well.  Copies of stored values: the comparisons are exact."""
import pytest
import torch

from embodied_clip_amd.dist import minibatch_bounds

pytestmark = pytest.mark.gpu

N, T, M = 8, 3, 3
COMMON = {"feat", "masks", "actions", "logp", "old_values", "returns", "advantages"}
AGENTS = {
    "rgbd": (dict(depth=True), {"feat2", "goal"}),
    "pooled": (dict(net="pooled", sensors=(2, 2), prev_actions=8), {"goal", "sensors", "prev_actions"}),
    "two_view": (dict(net="two_view"), {"feat2"}),
    "pointnav_il": (dict(goal_in=2, loss="ppo+imitation"), {"goal", "expert_actions", "expert_mask"}),
}


@pytest.mark.parametrize("name", sorted(AGENTS))
def test_gather_returns_the_rollout_storage_rows(name, monkeypatch):
    from embodied_clip_amd.engine import Worker
    kw, own = AGENTS[name]
    monkeypatch.setenv("EC_TWO_SLICE_MIN", "1")         # (the engine's switch: two slices below 48 actors)
    w = Worker(N, T=T, device="cuda:0", seed=0, num_mini_batch=M, **kw)
    assert w.ns == 2 and [(sl.o, sl.n) for sl in w.slices] == [(0, 4), (4, 4)]
    w.collect_rollout()
    w.compute_returns()
    w._gather_columns()
    torch.cuda.synchronize()
    env = w.env
    store = dict(feat=w.feat, feat2=w.feat2, goal=env.goals, sensors=getattr(env, "sensors", None), masks=env.masks,
                 actions=w.actions, logp=w.logp, old_values=w.values, returns=w.returns, advantages=w.nadv,
                 expert_actions=getattr(env, "expert_actions", None), expert_mask=getattr(env, "expert_mask", None),
                 prev_actions=w.prev_actions)
    inds = minibatch_bounds(N, M)
    assert list(inds) == [0, 3, 5, 8]
    parts = []
    for s0, s1 in zip(inds[:-1], inds[1:]):             # what update() forms
        for sl in w.slices:
            a, b = max(s0, sl.o) - sl.o, min(s1, sl.o + sl.n) - sl.o
            if b > a:
                parts.append((sl, a, b))
    assert [(sl.o, a, b) for sl, a, b in parts] == [(0, 0, 3), (0, 3, 4), (4, 0, 1), (4, 1, 4)]
    parts += [(sl, 0, sl.n) for sl in w.slices]         # ... and the whole slice
    for sl, a, b in parts:
        g = w.gather(sl, a, b)
        torch.cuda.synchronize()
        assert set(g) == COMMON | own, (name, sorted(g))
        m = b - a
        for col, got in g.items():
            want = store[col][:T, sl.o + a:sl.o + b]
            want = want.reshape((T * m,) + tuple(want.shape[2:]))
            assert got.is_contiguous() and got.shape == want.shape and got.dtype == want.dtype, (name, col, got.shape, want.shape)
            assert torch.equal(got, want), (name, col, sl.o, a, b)
        if (a, b) == (0, sl.n):                         # in place: no copy of the features
            assert g["feat"].data_ptr() == sl.feat.data_ptr()
    for sl in w.slices:                                 # staging holds the largest PARTIAL range (3 of the slice's 4 actors)
        assert w._max_partial_range(sl) == 3 < sl.n
        stages = [sl.feat_mb] + ([sl.feat2_mb] if w.feat2 is not None else [])
        for st in stages:
            assert st is not None and st.shape[:2] == (T, 3), tuple(st.shape)
        if w.feat2 is None:
            assert sl.feat2_mb is None
