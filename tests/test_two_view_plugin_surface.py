"""CPU: the plugin surface of the two-view rearrangement model -- ``ResNetRearrangeActorCriticRNN`` reached through upstream's
import path after ``install_into_allenact()``, its constructor's leading parameters, and the refusals of
``ec_nchw_f32_pair_to_nhwc_bf16`` (the one-launch conversion of both views), which come before any HIP call."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
    "rearrange/__init__.py": "",
    "rearrange/baseline_models.py": """
        class ResNetRearrangeActorCriticRNN: ORIGINAL = True
        class TwoPhaseRearrangeActorCriticSimpleConvRNN: ORIGINAL = True
        """,
    "rearrange_experiment_config.py": """
        from rearrange.baseline_models import ResNetRearrangeActorCriticRNN, TwoPhaseRearrangeActorCriticSimpleConvRNN
        """,
}


def test_rearrange_class_is_importable_through_the_upstream_path(tmp_path):
    for rel, src in FAKE_TREE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    prog = textwrap.dedent("""
        from embodied_clip_amd import allenact_compat as ac
        assert ac.HAVE_ALLENACT
        import allenact.algorithms.onpolicy_sync.policy as up_pol
        from embodied_clip_amd.policy import ResNetRearrangeActorCriticRNN, ResnetTensorObjectNavActorCritic
        assert issubclass(ResNetRearrangeActorCriticRNN, up_pol.ActorCriticModel)
        assert not issubclass(ResNetRearrangeActorCriticRNN, ResnetTensorObjectNavActorCritic)
        done = ac.install_into_allenact()
        assert 'rearrange.baseline_models.ResNetRearrangeActorCriticRNN' in done, done
        import rearrange_experiment_config as cfg         # imported AFTER the patch, as allenact_main does
        assert cfg.ResNetRearrangeActorCriticRNN is ResNetRearrangeActorCriticRNN
        assert not hasattr(cfg.ResNetRearrangeActorCriticRNN, 'ORIGINAL')
        assert cfg.TwoPhaseRearrangeActorCriticSimpleConvRNN.ORIGINAL      # (the two-phase model is not built: left alone)
        import inspect
        sig = inspect.signature(ResNetRearrangeActorCriticRNN.__init__).parameters
        kw = list(sig)[:8]
        assert kw == ['self', 'action_space', 'observation_space', 'rgb_uuid', 'unshuffled_rgb_uuid', 'hidden_size',
                      'num_rnn_layers', 'rnn_type'], kw
        assert (sig['hidden_size'].default, sig['num_rnn_layers'].default, sig['rnn_type'].default) == (512, 1, 'GRU')
        assert list(sig)[8:] == ['prev_action_embedding_dim', 'add_prev_action_null_token', 'attn_hidden', 'state_dict', 'device',
                                 'feature_rounding'], list(sig)[8:]
        assert sig['feature_rounding'].default == 'error' and sig['prev_action_embedding_dim'].default == 0
        print('OK', len(done))
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_module_is_bound_even_where_upstream_lacks_the_attribute(tmp_path):
    """treated like the other model modules: a ``rearrange.baseline_models`` without the class still gets it"""
    tree = dict(FAKE_TREE)
    tree["rearrange/baseline_models.py"] = "class SomethingElse: pass\n"
    del tree["rearrange_experiment_config.py"]
    for rel, src in tree.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    prog = textwrap.dedent("""
        from embodied_clip_amd import allenact_compat as ac
        done = ac.install_into_allenact()
        assert 'rearrange.baseline_models.ResNetRearrangeActorCriticRNN' in done, done
        from rearrange.baseline_models import ResNetRearrangeActorCriticRNN as got
        from embodied_clip_amd.policy import ResNetRearrangeActorCriticRNN
        assert got is ResNetRearrangeActorCriticRNN
        print('OK')
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_constructor_refusals():
    """ValueErrors raised before (or instead of) the handle's: they need no GPU"""
    import pytest
    from embodied_clip_amd import spaces
    from embodied_clip_amd.policy import ResNetRearrangeActorCriticRNN
    box = lambda *s: spaces.Box(-1e9, 1e9, s)
    obs = spaces.Dict({"rgb": box(64, 7, 7), "unshuffled_rgb": box(64, 7, 7), "other": box(64, 3, 3)})
    A = spaces.Discrete(84)
    with pytest.raises(ValueError, match="not in the observation space"):
        ResNetRearrangeActorCriticRNN(A, obs, "rgb", "missing", device="cpu")
    with pytest.raises(ValueError, match="same shape"):
        ResNetRearrangeActorCriticRNN(A, obs, "rgb", "other", device="cpu")
    for layers in (0, 5):
        with pytest.raises(ValueError, match="num_rnn_layers"):
            ResNetRearrangeActorCriticRNN(A, obs, "rgb", "unshuffled_rgb", num_rnn_layers=layers, device="cpu")
    with pytest.raises(ValueError, match="rnn_type"):
        ResNetRearrangeActorCriticRNN(A, obs, "rgb", "unshuffled_rgb", rnn_type="RNN", device="cpu")
    with pytest.raises(ValueError, match="feature_rounding"):
        ResNetRearrangeActorCriticRNN(A, obs, "rgb", "unshuffled_rgb", feature_rounding="truncate", device="cpu")


def test_pair_conversion_is_declared_bound_and_exported():
    from embodied_clip_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ec_amd.h")).read()
    assert re.search(r"\bint\s+ec_nchw_f32_pair_to_nhwc_bf16\s*\(", txt)
    res, args = _lib.SIGNATURES["ec_nchw_f32_pair_to_nhwc_bf16"]
    assert res is C.c_int and len(args) == 9 and args[4] is C.c_long            # B is a long
    assert hasattr(C.CDLL(_lib.LIB_PATH), "ec_nchw_f32_pair_to_nhwc_bf16")


def test_pair_conversion_refusals_come_before_any_hip_call():
    """dummy non-null pointers are never dereferenced on the host, and nothing is launched"""
    from embodied_clip_amd import _lib
    f = _lib.load().ec_nchw_f32_pair_to_nhwc_bf16
    EC_ERR_ARG, EC_ERR_SHAPE = -1, -2
    p = 4096
    for k in range(4):                                                          # a, b, out_a, out_b
        ptrs = [p] * 4
        ptrs[k] = None
        assert f(*ptrs, 1, 49, 64, p, None) == EC_ERR_ARG, k
        ptrs[k] = p + 8                                                         # not 16-byte aligned
        assert f(*ptrs, 1, 49, 64, p, None) == EC_ERR_ARG, k
    assert f(p, p, p, p, 1, 49, 64, None, None) == EC_ERR_ARG                  # changed
    assert f(p, p, p, p, 1, 49, 96, p, None) == EC_ERR_SHAPE                   # C % 64
    assert f(p, p, p, p, 1, 49, 0, p, None) == EC_ERR_SHAPE
    assert f(p, p, p, p, 1, 65, 64, p, None) == EC_ERR_SHAPE                   # HW outside 1..64
    assert f(p, p, p, p, 1, 0, 64, p, None) == EC_ERR_SHAPE
    assert f(p, p, p, p, 0, 49, 64, p, None) == EC_ERR_SHAPE                   # B <= 0
    assert f(p, p, p, p, -3, 49, 64, p, None) == EC_ERR_SHAPE
    assert f(p, p, p, p, 1 << 31, 49, 64, p, None) == EC_ERR_SHAPE             # more workgroups than a grid holds
