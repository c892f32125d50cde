"""Navigation metrics on the GPU: ``ec_nav_episode_stats`` against the sequential reference (tests/_nav_episode_ref.py), against
``ec_episode_stats`` on the columns the two share, and through ``Evaluator`` / ``Worker`` / the ``evaluate`` command line."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _episode_ref as er  # noqa: E402
from _child import GPU, last_json  # noqa: E402
import _nav_episode_ref as nr  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_COLS = (0, 3, 9)                 # episodes, sum length, no_path: integers, exact in any order
REC_I = ("actor", "t", "length", "category")
REC_F = ("return", "success", "spl", "soft_spl", "path", "goal_dist", "start_dist")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _random_calls(T, N, p=0.3, d_max=1.0, ids=12, calls=2):
    """Masks, rewards, success as ``_random_calls`` of test_gpu_eval.py builds them; geometry and goal ids on seeds of their own."""
    out = []
    for c in range(calls):
        ends = syn.hash_uniform(40 + c, T * N, stream=3).reshape(T, N) < p
        masks = np.ones((T + 1, N), dtype=np.float32)
        masks[1:][ends] = 0
        rewards = (syn.hash_uniform(50 + c, T * N, stream=4).reshape(T, N) * 2 - 1).astype(np.float32)
        success = ((syn.hash_uniform(60 + c, T * N, stream=5).reshape(T, N) < 0.5) & ends).astype(np.float32)
        step_dist, start_dist, goal_dist = (x.numpy() for x in syn.synthetic_navigation(70 + c, masks[1:], success, d_max=d_max))
        category = syn.synthetic_goals(80 + c, (T, N), ids).numpy()
        out.append((rewards, masks, success, step_dist, start_dist, goal_dist, category))
    return out


def _reference(calls, N, C, use=(True, True, True)):
    """``use``: (success, goal_dist, category) given or None."""
    ref = nr.NavEpisodeRef(N, C if use[2] else 0)
    for r, m, s, sd, d0, d1, cat in calls:
        ref.update(r, m, s if use[0] else None, sd, d0, d1 if use[1] else None, cat if use[2] else None)
    return ref


def _run_tracker(dev, calls, N, C, cap, use=(True, True, True)):
    from embodied_clip_amd.episodes import NavEpisodeTracker
    tr = NavEpisodeTracker(N, dev, num_categories=C if use[2] else 0, capacity=cap)
    g = lambda x: torch.from_numpy(x).to(dev)
    for r, m, s, sd, d0, d1, cat in calls:
        tr.update(g(r), g(m), g(s) if use[0] else None, g(sd), g(d0), g(d1) if use[1] else None, g(cat) if use[2] else None)
    torch.cuda.synchronize()
    return tr


def _check_totals(tot, ref):
    """Integer columns exact; every double sum within n * 2^-53 * sum|x| of the correctly rounded one, n the row's episodes."""
    want, scale = ref.totals(), ref.abs_sums()
    assert len(tot) == len(want)
    for r, (got_row, want_row, abs_row) in enumerate(zip(tot, want, scale)):
        n = want_row[0]
        for i in range(10):
            bound = 0.0 if i in INT_COLS else n * U * abs_row[i]
            if abs(got_row[i] - want_row[i]) > bound:
                print("row", r, nr.COLS[i], "got", got_row[i], "want", want_row[i], "bound", bound)
            assert abs(got_row[i] - want_row[i]) <= bound, (r, nr.COLS[i])


def _check_against_ref(tr, ref, cap):
    tot = tr.totals.tolist()
    print("row 0", tot[0], "ref", ref.totals()[0])
    _check_totals(tot, ref)
    n = len(ref.records)
    assert int(tr.n_records.item()) == n             # advances past cap: the overflow is visible
    rec = tr.records()
    k = min(n, cap)
    assert rec["dropped"] == n - k
    want = ref.records[:k]
    for key in REC_I:
        assert torch.equal(rec[key].cpu(), torch.tensor([r[key] for r in want], dtype=torch.int32)), key
    for key in REC_F:
        got, exp = rec[key].cpu(), torch.tensor([float(r[key]) for r in want], dtype=torch.float32)
        if not torch.equal(got, exp):
            bad = (got != exp).nonzero().flatten().tolist()
            print(key, "differs at", bad[:8], got[bad[:8]].tolist(), exp[bad[:8]].tolist())
        assert torch.equal(got, exp), key
    assert torch.equal(tr.carry_ret.cpu(), torch.from_numpy(ref.carry_ret))
    assert torch.equal(tr.carry_len.cpu(), torch.from_numpy(ref.carry_len))
    assert torch.equal(tr.carry_path.cpu(), torch.from_numpy(ref.carry_path))


def _check_rows_add_up(tot, ref):
    """Rows 1..C against row 0: exact in the integer columns, within the summation bound in the others."""
    scale = ref.abs_sums()[0]
    n = ref.totals()[0][0]
    for i in range(10):
        s = math.fsum(r[i] for r in tot[1:])
        assert abs(s - tot[0][i]) <= (0.0 if i in INT_COLS else n * U * scale[i]), nr.COLS[i]


# ---- 1. the hand-made case ----------------------------------------------------------------------------------------------------

def test_hand_made_case(dev):
    calls = nr.hand_case()
    ref = _reference(calls, er.HAND_N, nr.HAND_C)
    tr = _run_tracker(dev, calls, er.HAND_N, nr.HAND_C, cap=16)
    _check_against_ref(tr, ref, 16)
    rec = tr.records()
    assert rec["path"].tolist() == nr.HAND_PATH and rec["spl"].tolist() == nr.HAND_SPL
    assert rec["soft_spl"].tolist() == nr.HAND_SOFT_SPL and rec["category"].tolist() == nr.HAND_CATEGORY
    assert tr.carry_path.tolist() == nr.HAND_CARRY_PATH and tr.carry_len.tolist() == er.HAND_CARRY_LEN
    again = _run_tracker(dev, calls, er.HAND_N, nr.HAND_C, cap=16)
    assert torch.equal(tr.totals, again.totals)
    info, want = tr.info(), ref.info()
    assert info["episodes"] == 7 and info["no_path"] == 1
    for key in want:
        assert info[key] == pytest.approx(want[key], rel=1e-12), key
    assert tr.info_by_category()["1"]["episodes"] == 3 and tr.info_by_category(["a", "b", "c"])["b"]["no_path"] == 1
    tr.reset()
    assert tr.info()["episodes"] == 0 and np.isnan(tr.info()["spl"]) and tr.carry_path.tolist() == nr.HAND_CARRY_PATH


# ---- 2. more actors than a block ----------------------------------------------------------------------------------------------

WIDE_T, WIDE_N, WIDE_C = 3, 1030, 12


@pytest.fixture(scope="module")
def wide_case():
    calls = _random_calls(WIDE_T, WIDE_N)
    return calls, _reference(calls, WIDE_N, WIDE_C)


def test_wide_case_covers_the_branches(wide_case):
    """The floors of what the reference run must contain for the comparisons below to mean something (needs no GPU work)."""
    calls, ref = wide_case
    r = ref.records
    assert sum(1 for x in r if x["success"] > 0 and x["start_dist"] > 0 and x["spl"] < 1) >= 50
    assert sum(1 for x in r if x["start_dist"] == 0) >= 10
    assert sum(1 for x in r if x["start_dist"] < 0) >= 10
    assert min(row[0] for row in ref.totals()[1:]) >= 50
    assert any(x["actor"] >= 1024 for x in r)
    assert len(ref.calls[0]) > 100                                   # cap = 100 overflows inside the first call
    assert sum(1 for x in ref.calls[1] if x["length"] > x["t"] + 1) >= 50      # episodes that cross the call boundary
    assert sum(1 for x in r if x["soft_spl"] > 0) >= 50 and sum(1 for x in r if x["soft_spl"] == 0) >= 50


@pytest.mark.parametrize("cap", [2000, 100])
def test_more_actors_than_a_block(dev, wide_case, cap):
    calls, ref = wide_case
    tr = _run_tracker(dev, calls, WIDE_N, WIDE_C, cap)
    _check_against_ref(tr, ref, cap)
    _check_rows_add_up(tr.totals.tolist(), ref)
    again = _run_tracker(dev, calls, WIDE_N, WIDE_C, cap)
    assert torch.equal(tr.totals, again.totals) and torch.equal(tr.rec_f, again.rec_f) and torch.equal(tr.rec_i, again.rec_i)


# ---- 3. ids out of range, absent inputs ---------------------------------------------------------------------------------------

def test_out_of_range_ids_and_absent_inputs(dev):
    T, N, C = 6, 70, 12
    calls = _random_calls(T, N, ids=14)
    ref = _reference(calls, N, C)
    outside = sum(1 for x in ref.records if x["category"] >= C)
    assert outside >= 10 and {12, 13} <= {x["category"] for x in ref.records}
    tr = _run_tracker(dev, calls, N, C, cap=400)
    _check_against_ref(tr, ref, 400)                                 # (the records keep ids 12 and 13 as given)
    tot = tr.totals.tolist()
    assert tot[0][0] - sum(r[0] for r in tot[1:]) == outside         # ... and the rows miss exactly those episodes
    # no categories: one row.  The kernel gathers row 0 in the lanes' registers and folds it with the fixed-order block sum,
    # whatever C is, so it GUARANTEES the bits of row 0 of the run with categories
    bare = _run_tracker(dev, calls, N, C, cap=400, use=(True, True, False))
    assert tuple(bare.totals.shape) == (1, 10) and torch.equal(bare.totals[0], tr.totals[0])
    assert (bare.records()["category"] == -1).all()
    _check_against_ref(bare, _reference(calls, N, C, (True, True, False)), 400)
    # no distance to the goal: nothing accumulated, NaN reported
    nogoal = _run_tracker(dev, calls, N, C, cap=400, use=(True, False, True))
    _check_against_ref(nogoal, _reference(calls, N, C, (True, False, True)), 400)
    assert (nogoal.totals[:, 6] == 0).all() and (nogoal.totals[:, 7] == 0).all()
    info = nogoal.info()
    assert np.isnan(info["soft_spl"]) and np.isnan(info["dist_to_goal"]) and info["spl"] > 0 and info["path_length"] > 0
    assert np.isnan(nogoal.info_by_category()["3"]["soft_spl"])
    assert torch.equal(nogoal.totals[:, :6], tr.totals[:, :6]) and torch.equal(nogoal.totals[:, 8:], tr.totals[:, 8:])
    # no success flags: spl 0 everywhere (soft_spl does not read them)
    nosucc = _run_tracker(dev, calls, N, C, cap=400, use=(False, True, True))
    _check_against_ref(nosucc, _reference(calls, N, C, (False, True, True)), 400)
    assert (nosucc.totals[:, 5] == 0).all() and (nosucc.records()["spl"] == 0).all() and nosucc.info()["spl"] == 0
    from embodied_clip_amd.episodes import NavEpisodeTracker
    with pytest.raises(ValueError):
        NavEpisodeTracker(N, dev, num_categories=0).update(*[torch.from_numpy(x).to(dev) for x in calls[0]])
    with pytest.raises(ValueError):
        NavEpisodeTracker(N, dev, num_categories=65)


# ---- 4. against ec_episode_stats ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [2000])
def test_shared_columns_equal_the_plain_tracker(dev, wide_case, cap):
    from embodied_clip_amd.episodes import EpisodeTracker
    calls, ref = wide_case
    tr = _run_tracker(dev, calls, WIDE_N, WIDE_C, cap)
    plain = EpisodeTracker(WIDE_N, dev, capacity=cap)
    for r, m, s, *_ in calls:
        plain.update(torch.from_numpy(r).to(dev), torch.from_numpy(m).to(dev), torch.from_numpy(s).to(dev))
    torch.cuda.synchronize()
    a, b = tr.totals[0].tolist(), plain.totals.tolist()
    n, scale = ref.totals()[0][0], ref.abs_sums()[0]
    assert a[0] == b[0] == n and a[3] == b[3] and a[4] == b[4]
    assert abs(a[1] - b[1]) <= n * U * scale[1] and abs(a[2] - b[2]) <= n * U * scale[2]
    for key in ("actor", "t", "length", "return", "success"):
        assert torch.equal(tr.records()[key], plain.records()[key]), key
    assert torch.equal(tr.carry_ret, plain.carry_ret) and torch.equal(tr.carry_len, plain.carry_len)


# ---- 5. long episodes ---------------------------------------------------------------------------------------------------------

def test_long_episodes(dev):
    T, N, C = 128, 8, 3
    calls = _random_calls(T, N, p=0.05, d_max=4.0, ids=C)
    ref = _reference(calls, N, C)
    r = ref.records
    assert len(r) >= 50 and sum(1 for x in r if 0 < x["spl"] < 1) >= 10 and max(x["length"] for x in r) >= 40
    assert sum(1 for x in ref.calls[1] if x["length"] > x["t"] + 1) >= 4
    tr = _run_tracker(dev, calls, N, C, cap=256)
    _check_against_ref(tr, ref, 256)
    _check_rows_add_up(tr.totals.tolist(), ref)


# ---- 6. through the engine ----------------------------------------------------------------------------------------------------

ENG_N, ENG_T = 4, 3
ENG_ENDS = [(0, 0), (2, 0), (1, 1), (2, 3)]          # (t, n): actor 0 twice a chunk, actor 2 never
ENG_WINS = [(0, 0), (2, 3)]                          # ... and two of the four ends succeed


def _end_episodes(env):
    masks = torch.ones_like(env.masks)
    for t, n in ENG_ENDS:
        masks[t + 1, n] = 0
    env.masks.copy_(masks)
    env.success.zero_()
    for t, n in ENG_WINS:
        env.success[t, n] = 1


def _env_reference(env, chunks):
    C = env.num_goals
    ref = nr.NavEpisodeRef(env.N, C)
    f = lambda x: x.cpu().numpy()
    for _ in range(chunks):
        ref.update(f(env.rewards), f(env.masks), f(env.success), f(env.step_dist), f(env.start_dist), f(env.goal_dist), f(env.goals))
    return ref


@pytest.fixture(scope="module")
def enc_sd():
    return syn.rn50_visual_state_dict(0)


def test_metrics_through_evaluator_and_worker(dev, enc_sd):
    from embodied_clip_amd.engine import NavSyntheticEnv, SyntheticEnv, Worker
    from embodied_clip_amd.evaluate import Evaluator
    N, T = ENG_N, ENG_T
    env = NavSyntheticEnv(N, T, dev, seed=1000, goal_in=0)
    plain_env = SyntheticEnv(N, T, dev, seed=1000)
    for key in ("frames", "masks", "goals", "rewards", "success"):     # the subclass adds tensors and changes none
        assert torch.equal(getattr(env, key), getattr(plain_env, key)), key
    assert env.num_goals == 12 and tuple(env.step_dist.shape) == tuple(env.start_dist.shape) == tuple(env.goal_dist.shape) == (T, N)
    _end_episodes(env)
    want = _env_reference(env, 2).info()
    assert want["episodes"] == 8 and want["success"] == 0.5 and want["spl"] > 0
    ev = Evaluator(N, T=T, device="cuda:0", seed=2, encoder_sd=enc_sd, env=env, record_capacity=64, nav_metrics=True, record=True)
    assert ev.episodes.C == 12 and np.isnan(ev.info()["spl"])
    ev.run(2)
    torch.cuda.synchronize()
    info = ev.info()
    print("evaluator info", info, "reference", want)
    assert set(info) == set(want)
    for key in want:
        if key in ("episodes", "no_path"):
            assert info[key] == want[key], key
        else:
            assert info[key] == pytest.approx(want[key], rel=1e-12), key
    assert ev.episodes.records()["dropped"] == 0 and len(ev.episodes.records()["spl"]) == 8
    assert sum(v["episodes"] for v in ev.episodes.info_by_category().values()) == 8
    # the plain evaluator on the same env: the same five keys, the same actions
    env._k = 0                                # (the env serves its frames from the start again)
    base = Evaluator(N, T=T, device="cuda:0", seed=2, encoder_sd=enc_sd, env=env, record_capacity=64, record=True)
    base.run(2)
    torch.cuda.synchronize()
    assert {k: info[k] for k in base.info()} == base.info()
    assert torch.equal(base.actions, ev.actions) and torch.equal(base.logp, ev.logp) and torch.equal(base.hv, ev.hv)
    del ev, base
    w = Worker(N, T=T, device="cuda:0", seed=2, update_repeats=1, encoder_sd=enc_sd, track_episodes=True, nav_metrics=True)
    assert torch.equal(w.env.step_dist, env.step_dist) and torch.equal(w.env.goals, env.goals)
    _end_episodes(w.env)
    w.iteration()
    w.iteration()
    torch.cuda.synchronize()
    assert w.episode_info() == info
    with pytest.raises(ValueError, match="track_episodes"):
        Worker(N, T=T, device="cuda:0", nav_metrics=True)


def test_coordinate_goals_have_no_categories(dev, enc_sd):
    from embodied_clip_amd.evaluate import Evaluator
    ev = Evaluator(ENG_N, T=ENG_T, device="cuda:0", seed=2, encoder_sd=enc_sd, goal_in=2, num_actions=4, nav_metrics=True)
    assert ev.episodes.C == 0 and ev.env.num_goals == 0 and tuple(ev.episodes.totals.shape) == (1, 10)
    _end_episodes(ev.env)
    info = ev.run(1)
    assert info["episodes"] == 4 and 0 <= info["spl"] <= 1 and ev.episodes.info_by_category() == {}


def test_env_without_geometry_is_refused(dev):
    from embodied_clip_amd.engine import NavSyntheticEnv, SyntheticEnv
    from embodied_clip_amd.evaluate import Evaluator
    with pytest.raises(ValueError, match="step_dist"):
        Evaluator(ENG_N, T=ENG_T, device="cuda:0", env=SyntheticEnv(ENG_N, ENG_T, dev, seed=1000), nav_metrics=True)
    env = NavSyntheticEnv(ENG_N, ENG_T, dev, seed=1000)
    del env.start_dist
    with pytest.raises(ValueError, match="start_dist"):
        Evaluator(ENG_N, T=ENG_T, device="cuda:0", env=env, nav_metrics=True)


def test_goal_dist_is_optional(dev, enc_sd):
    from embodied_clip_amd.engine import NavSyntheticEnv
    from embodied_clip_amd.evaluate import Evaluator
    env = NavSyntheticEnv(ENG_N, ENG_T, dev, seed=1000)
    del env.goal_dist
    _end_episodes(env)
    ev = Evaluator(ENG_N, T=ENG_T, device="cuda:0", seed=2, encoder_sd=enc_sd, env=env, nav_metrics=True)
    info = ev.run(1)
    assert info["episodes"] == 4 and np.isnan(info["soft_spl"]) and np.isnan(info["dist_to_goal"]) and not np.isnan(info["spl"])


def test_command_line_writes_the_metrics_file(dev, tmp_path):
    """The CLI in a child process; this project's reader of the metrics file reproduces the printed per-object-type scores."""
    from embodied_clip_amd.evaluate import scores_by_object_type
    env_seed = 1073                           # the synthetic masks of this seed end two episodes in a 3-step chunk of 4 actors
    assert int((syn.synthetic_masks(env_seed + 1, 3, 4) == 0).sum()) == 2
    fixture = os.path.join(REPO, "tests", "golden", "robothor_object_types.json")
    names = json.load(open(fixture))["object_types"]
    out = str(tmp_path / "metrics.json")
    res = GPU.run([sys.executable, "-m", "embodied_clip_amd.evaluate", "--actors", "4", "--steps", "3", "--chunks", "2",
                   "--env-seed", str(env_seed), "--nav-metrics", "--object-types", fixture, "--groups", fixture,
                   "--metrics-json", out], cwd=REPO, limit=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = last_json(res)
    assert line["episodes"] == 4 and set(line["by_object_type"]) == set(names) and set(line["groups"]) == {"seen", "unseen"}
    for key in ("spl", "soft_spl", "dist_to_goal", "path_length"):
        assert key in line
    metrics = json.load(open(out))
    assert len(metrics) == 1 and len(metrics[0]["tasks"]) == 4 and "dropped" not in metrics[0]
    scores = scores_by_object_type(out, names)
    seen_types = 0
    for name in names:
        want = line["by_object_type"][name]
        if want["episodes"] == 0:
            assert np.isnan(scores[name][0]) and np.isnan(scores[name][1])
        else:
            seen_types += 1
            assert scores[name][0] == pytest.approx(want["success"], rel=1e-12)
            assert scores[name][1] == pytest.approx(want["spl"], rel=1e-12, abs=1e-300)
    assert seen_types >= 1
    assert line["groups"]["seen"]["episodes"] + line["groups"]["unseen"]["episodes"] == 4
