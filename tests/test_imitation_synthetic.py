"""The synthetic expert, the env's expert tensors, the teacher-forcing schedules and the AllenAct rebind (no GPU)."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from embodied_clip_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expert_is_deterministic_and_in_range():
    goals = syn.synthetic_goals(5, (9, 7))
    a, m = syn.synthetic_expert(3, goals, 6)
    a2, m2 = syn.synthetic_expert(3, goals, 6)
    assert torch.equal(a, a2) and torch.equal(m, m2)
    assert a.dtype == torch.int64 and m.dtype == torch.float32 and a.shape == m.shape == goals.shape
    assert torch.equal(a, goals % 6)                           # a function of the goal alone
    assert set(m.unique().tolist()) <= {0.0, 1.0}
    # 84 actions (the rearrangement action space): ids stay below the number of goals, in range
    a84, _ = syn.synthetic_expert(3, goals, 84)
    assert int(a84.min()) >= 0 and int(a84.max()) < 84
    # coordinate goals: the bearing's sector
    gv = syn.synthetic_goal_vectors(5, (9, 7), 2)
    av, mv = syn.synthetic_expert(3, gv, 4)
    assert av.shape == mv.shape == (9, 7) and int(av.min()) >= 0 and int(av.max()) < 4
    assert len(av.unique()) == 4
    same = (gv[..., 1] >= 0) & (gv[..., 1] < 3.14159 / 2)      # bearing in [0, pi/2): the third of four sectors
    assert torch.all(av[same] == 2)
    # p_fail: 0 never fails; the mask's stream does not depend on the goals
    assert torch.all(syn.synthetic_expert(3, goals, 6, p_fail=0.0)[1] == 1)
    assert torch.equal(mv, m)


def test_mask_has_both_values_at_the_gpu_tests_shapes():
    """The engine tests run rollouts of a few steps: they install ``engine_test_mask`` (p_fail 0.3), which holds both values at
    each of their shapes; the env's own mask (p_fail 0.05; Worker(seed=3) builds it from seed 1006) does from ~100 steps on."""
    import _imitation_ref as ref
    for T, N in ref.ENGINE_SHAPES:
        m = ref.engine_test_mask(T, N)
        assert m.shape == (T + 1, N) and 0 < int((m[:T] == 0).sum()) < T * N, (T, N)
    _, m = syn.synthetic_expert(1006, syn.synthetic_goals(1002, (5, 64)), 6)
    assert 0 < int((m[:4] == 0).sum()) < 4 * 64


def test_env_without_expert_is_unchanged():
    from embodied_clip_amd.engine import NavSyntheticEnv, SyntheticEnv
    for cls in (SyntheticEnv, NavSyntheticEnv):
        e0 = cls(3, 4, "cpu", seed=1000, res=8)
        e1 = cls(3, 4, "cpu", seed=1000, res=8, expert=True, num_actions=6)
        for k in ("frames", "masks", "goals", "rewards", "success"):
            assert torch.equal(getattr(e0, k), getattr(e1, k)), k
        assert not hasattr(e0, "expert_actions") and not hasattr(e0, "expert_mask")
        assert e1.expert_actions.shape == e1.expert_mask.shape == (5, 3)
        assert torch.equal(e1.expert_actions, e1.goals % 6)
        # today's tensors, restated from the generators
        assert torch.equal(e0.goals, syn.synthetic_goals(1002, (5, 3)))
        assert torch.equal(e0.masks[1:], syn.synthetic_masks(1001, 4, 3).reshape(4, 3))
    ev = SyntheticEnv(3, 4, "cpu", seed=1000, res=8, goal_in=2, expert=True, num_actions=4)
    assert torch.equal(ev.goals, syn.synthetic_goal_vectors(1002, (5, 3), 2)) and int(ev.expert_actions.max()) < 4


def test_schedules():
    from embodied_clip_amd.imitation import LinearDecay, StepwiseLinearDecay
    ld = LinearDecay(steps=1000)
    assert ld(0) == 1.0 and ld(1000) == 0.0 and ld(5000) == 0.0 and ld(-5) == 1.0
    assert ld(250) == pytest.approx(0.75) and ld(500) == pytest.approx(0.5)
    ld2 = LinearDecay(steps=10, startp=0.2, endp=0.8)
    assert ld2(0) == pytest.approx(0.2) and ld2(5) == pytest.approx(0.5) and ld2(10) == pytest.approx(0.8)
    sw = StepwiseLinearDecay([(0, 1.0), (100, 1.0), (300, 0.5), (400, 0.0)])
    assert sw(0) == 1.0 and sw(50) == 1.0 and sw(100) == 1.0
    assert sw(200) == pytest.approx(0.75) and sw(300) == pytest.approx(0.5)
    assert sw(350) == pytest.approx(0.25) and sw(400) == 0.0 and sw(10 ** 9) == 0.0
    assert StepwiseLinearDecay([(400, 0.0), (0, 1.0)])(100) == pytest.approx(0.75)      # sorted on construction
    assert StepwiseLinearDecay([(10, 0.3)])(0) == 0.3


def test_loss_refuses_what_is_not_implemented():
    from embodied_clip_amd.imitation import Imitation
    with pytest.raises(NotImplementedError, match="expert_policy"):
        Imitation().loss(0, {"observations": {"expert_policy": torch.zeros(2, 2, 7)}}, None)
    with pytest.raises(NotImplementedError, match="expert_action"):
        Imitation().loss(0, {"observations": {"rgb": torch.zeros(2)}}, None)


FAKE_TREE = {
    "allenact/__init__.py": "",
    "allenact/base_abstractions/__init__.py": "",
    "allenact/base_abstractions/misc.py": """
        class Memory(dict): pass
        class ActorCriticOutput(tuple):
            def __new__(cls, distributions, values, extras): return super().__new__(cls, (distributions, values, extras))
        """,
    "allenact/base_abstractions/distributions.py": """
        import torch
        class CategoricalDistr(torch.distributions.Categorical): pass
        """,
    "allenact/base_abstractions/preprocessor.py": """
        class Preprocessor:
            def __init__(self, input_uuids, output_uuid, observation_space, **kwargs):
                self.uuid, self.input_uuids, self.observation_space = output_uuid, input_uuids, observation_space
        """,
    "allenact/algorithms/__init__.py": "",
    "allenact/algorithms/onpolicy_sync/__init__.py": "",
    "allenact/algorithms/onpolicy_sync/policy.py": """
        import torch.nn as nn
        class ActorCriticModel(nn.Module):
            def __init__(self, action_space, observation_space):
                super().__init__(); self.action_space, self.observation_space = action_space, observation_space
        """,
    "allenact/algorithms/onpolicy_sync/losses/__init__.py": """
        from allenact.algorithms.onpolicy_sync.losses.imitation import Imitation
        """,
    "allenact/algorithms/onpolicy_sync/losses/abstract_loss.py": """
        class AbstractActorCriticLoss:
            MARK = 'fake-allenact'
            def __init__(self, *a, **k): pass
        """,
    "allenact/algorithms/onpolicy_sync/losses/imitation.py": """
        class Imitation: ORIGINAL = True
        """,
    "imitation_experiment_config.py": """
        from allenact.algorithms.onpolicy_sync.losses import Imitation
        from allenact.algorithms.onpolicy_sync.losses.imitation import Imitation as Imitation2
        """,
}


def test_install_into_allenact_rebinds_imitation(tmp_path):
    for rel, src in FAKE_TREE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    prog = textwrap.dedent("""
        from embodied_clip_amd import allenact_compat as ac
        assert ac.HAVE_ALLENACT
        from embodied_clip_amd.imitation import Imitation
        assert Imitation.MARK == 'fake-allenact'              # the real ABC when allenact is importable
        done = ac.install_into_allenact()
        assert 'allenact.algorithms.onpolicy_sync.losses.imitation.Imitation' in done, done
        assert 'allenact.algorithms.onpolicy_sync.losses.Imitation' in done, done
        import imitation_experiment_config as cfg            # imported AFTER the patch, as allenact_main does
        assert cfg.Imitation is Imitation and cfg.Imitation2 is Imitation
        assert not hasattr(cfg.Imitation, 'ORIGINAL')
        print('OK', len(done))
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
