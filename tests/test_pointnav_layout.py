"""CPU: the PointNav handle (``ec_policy_cfg.goal_in > 0``) -- flat layout, workspace sizes, refusals, synthetic
parameters and the AllenAct import path.  None of these entry points makes a HIP call (as in test_policy_layout.py)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from embodied_clip_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTNAV_PARAMS = 3_479_461       # 3,480,775 - 384 (embed_class) + 96 (embed_goal) - 1,026 (actor 6 -> 4)


def _create(**cfg):
    from embodied_clip_amd import _lib
    lib = _lib.load()
    full = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6, compress_hid=128,
                compress_out=32, comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0)
    full.update(cfg)
    h = C.c_void_p()
    rc = lib.ec_policy_create(C.byref(h), C.byref(_lib.PolicyCfg(**full)))
    return lib, h, rc


def _layout(lib, h):
    out = []
    for i in range(lib.ec_policy_num_param_tensors(h)):
        off, num = C.c_size_t(), C.c_size_t()
        assert lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)) == 0
        out.append((off.value, num.value))
    return out


def test_pointnav_flat_layout_default_geometry():
    lib, h, rc = _create(goal_in=2, num_actions=4)
    assert rc == 0
    try:
        lay = _layout(lib, h)
        shapes = syn.policy_param_shapes(goal_in=2, num_actions=4)
        assert len(lay) == 18 and list(shapes) == list(syn.policy_param_order(goal_in=2))
        # embed_goal.weight [goal_dims, goal_in] and embed_goal.bias [goal_dims] first, then the 16 others in today's order
        assert list(shapes)[:2] == ["goal_visual_encoder.embed_goal.weight", "goal_visual_encoder.embed_goal.bias"]
        assert list(shapes)[2:] == list(syn.POLICY_PARAM_ORDER[1:])
        want = [int(torch.Size(s).numel()) for s in shapes.values()]
        assert [n for _, n in lay] == want and want[:2] == [64, 32]
        assert sum(want) == POINTNAV_PARAMS
        offs = [o for o, _ in lay]
        assert offs == sorted(offs) and offs[0] == 0 and all(o % 4 == 0 for o in offs)       # 16-byte aligned (fp32)
        assert all(o1 >= o0 + n0 for (o0, n0), (o1, _) in zip(lay, lay[1:]))                  # no overlap
        assert lib.ec_policy_flat_size(h) >= sum(want)
    finally:
        lib.ec_policy_destroy(h)


def test_goal_in_3_adds_exactly_32_floats():
    lib, h2, rc2 = _create(goal_in=2, num_actions=4)
    _, h3, rc3 = _create(goal_in=3, num_actions=4)
    assert rc2 == 0 and rc3 == 0
    try:
        n2, n3 = sum(n for _, n in _layout(lib, h2)), sum(n for _, n in _layout(lib, h3))
        assert n3 - n2 == 32
        assert _layout(lib, h3)[0][1] == 96
    finally:
        lib.ec_policy_destroy(h2)
        lib.ec_policy_destroy(h3)


def test_pointnav_workspace_sizes():
    lib, h, rc = _create(goal_in=2, num_actions=4)
    assert rc == 0
    try:
        for T, N in ((1, 1), (1, 37), (4, 8), (128, 2)):
            act, learn = lib.ec_policy_workspace_bytes(h, T, N, 0), lib.ec_policy_workspace_bytes(h, T, N, 1)
            assert 0 < act < learn, (T, N, act, learn)
    finally:
        lib.ec_policy_destroy(h)


def test_goal_in_refusals():
    from embodied_clip_amd import _lib
    EC_ERR_ARG, EC_ERR_UNSUPPORTED = -1, -6
    lib, h, rc = _create(goal_in=2, fusion=1, spatial=1, in_channels=1024)
    assert rc == EC_ERR_ARG and not h.value
    assert _create(goal_in=9)[2] == EC_ERR_ARG and _create(goal_in=-1)[2] == EC_ERR_ARG
    assert _create(goal_in=2, dual=1)[2] == EC_ERR_UNSUPPORTED          # the RGB-D PointNav encoder is not built (ec_amd.h)
    lib, h, rc = _create(goal_in=2, num_goals=0)                          # num_goals is ignored with goal_in > 0
    assert rc == 0
    lib.ec_policy_destroy(h)
    assert _lib.PolicyCfg(in_channels=1).goal_in == 0                     # cfgs that carry no goal_in: zero-filled


def test_wrong_goal_type_entry_points_are_refused():
    """The integer entry points return EC_ERR_ARG on a goal_in > 0 handle, the vector ones on a goal_in == 0 handle -- checked
    before anything is launched (dummy non-null pointers are never dereferenced on the host)."""
    EC_ERR_ARG = -1
    p = C.c_void_p(4096)
    for goal_in, fwd, act in ((2, "ec_policy_forward2", "ec_policy_act"), (0, "ec_policy_forward_vec", "ec_policy_act_vec")):
        lib, h, rc = _create(goal_in=goal_in, num_actions=4)
        assert rc == 0
        try:
            assert getattr(lib, fwd)(h, p, p, None, 1, p, p, p, 1, 1, p, 1 << 30, 0, p, p, None) == EC_ERR_ARG
            assert getattr(lib, act)(h, p, p, None, 1, p, p, p, 1, p, 1 << 30, 0, p, p, p, p, p, 0, 0, 0, None) == EC_ERR_ARG
        finally:
            lib.ec_policy_destroy(h)


def test_pointnav_state_dict_names_and_init():
    sd = syn.policy_state_dict(0, goal_in=2, num_actions=4)
    assert list(sd) == list(syn.policy_param_order(goal_in=2)) and len(sd) == 18
    assert not any("embed_class" in k for k in sd)
    w, b = sd["goal_visual_encoder.embed_goal.weight"], sd["goal_visual_encoder.embed_goal.bias"]
    assert tuple(w.shape) == (32, 2) and tuple(b.shape) == (32,)
    assert sd["actor.linear.weight"].shape == (4, 512)
    assert sum(v.numel() for v in sd.values()) == POINTNAV_PARAMS
    w8 = syn.policy_state_dict(0, goal_in=8)["goal_visual_encoder.embed_goal.weight"]      # N(0, 1/goal_in)
    assert abs(float(w8.std()) - 8 ** -0.5) < 0.15 * 8 ** -0.5 and abs(float(w.std()) - 2 ** -0.5) < 0.3 * 2 ** -0.5
    g = syn.synthetic_goal_vectors(3, (5, 7), 3)
    assert g.shape == (5, 7, 3) and g.dtype == torch.float32
    assert 0 <= float(g[..., 0].min()) and float(g[..., 0].max()) < 10
    assert -3.1416 <= float(g[..., 1:].min()) and float(g[..., 1:].max()) < 3.1416 and float(g[..., 1:].min()) < 0
    assert torch.equal(g, syn.synthetic_goal_vectors(3, (5, 7), 3))
    from embodied_clip_amd.policy import PolicyHandle
    h = PolicyHandle(goal_in=2, num_actions=4)
    assert list(h.offsets) == list(sd) and h.goal_in == 2
    rec = h.recurrent_section()
    assert rec.start == h.offsets["state_encoder.rnn.weight_ih_l0"][0] and rec.stop == h.flat_size


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
            MARK = 'fake-allenact'
            def __init__(self, action_space, observation_space):
                super().__init__(); self.action_space, self.observation_space = action_space, observation_space
        """,
    "allenact/algorithms/onpolicy_sync/losses/__init__.py": "",
    "allenact/algorithms/onpolicy_sync/losses/abstract_loss.py": """
        class AbstractActorCriticLoss:
            def __init__(self, *a, **k): pass
        """,
    "projects/__init__.py": "",
    "projects/pointnav_baselines/__init__.py": "",
    "projects/pointnav_baselines/models/__init__.py": "",
    "projects/pointnav_baselines/models/point_nav_models.py": """
        class ResnetTensorPointNavActorCritic: ORIGINAL = True
        """,
    "pointnav_experiment_config.py": """
        from projects.pointnav_baselines.models.point_nav_models import ResnetTensorPointNavActorCritic
        """,
}


def test_pointnav_class_is_importable_through_the_upstream_path(tmp_path):
    for rel, src in FAKE_TREE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    prog = textwrap.dedent("""
        from embodied_clip_amd import allenact_compat as ac
        assert ac.HAVE_ALLENACT
        import allenact.algorithms.onpolicy_sync.policy as up_pol
        from embodied_clip_amd.policy import ResnetTensorObjectNavActorCritic, ResnetTensorPointNavActorCritic
        assert issubclass(ResnetTensorPointNavActorCritic, up_pol.ActorCriticModel)
        assert not issubclass(ResnetTensorPointNavActorCritic, ResnetTensorObjectNavActorCritic)
        done = ac.install_into_allenact()
        assert 'projects.pointnav_baselines.models.point_nav_models.ResnetTensorPointNavActorCritic' in done, done
        import pointnav_experiment_config as cfg         # imported AFTER the patch, as allenact_main does
        assert cfg.ResnetTensorPointNavActorCritic is ResnetTensorPointNavActorCritic
        assert not hasattr(cfg.ResnetTensorPointNavActorCritic, 'ORIGINAL')
        import inspect
        kw = list(inspect.signature(ResnetTensorPointNavActorCritic.__init__).parameters)[1:10]
        assert kw == ['action_space', 'observation_space', 'goal_sensor_uuid', 'rgb_resnet_preprocessor_uuid',
                      'depth_resnet_preprocessor_uuid', 'hidden_size', 'goal_dims', 'resnet_compressor_hidden_out_dims',
                      'combiner_hidden_out_dims'], kw
        print('OK', len(done))
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
