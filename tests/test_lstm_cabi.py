"""The LSTM core on a box without a GPU: the new symbols declared, exported and bound; ``ec_policy_create_rnn(.., EC_RNN_GRU)`` is
today's handle (the golden layout); the LSTM layout; every refusal in front of the first HIP call."""
import ctypes as C
import json
import os
import re

import pytest

NEW = ("ec_policy_create_rnn", "ec_policy_rnn_type", "ec_policy_state_width", "ec_lstm_step_fwd", "ec_lstm_step_bwd")
REFERENCE = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6, compress_hid=128, compress_out=32,
                 comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0)
GRU, LSTM = 0, 1
RNN = ("state_encoder.rnn.weight_ih_l0", "state_encoder.rnn.weight_hh_l0", "state_encoder.rnn.bias_ih_l0", "state_encoder.rnn.bias_hh_l0")
P = 64        # a non-NULL "pointer": the checks under test return before anything is read


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def _create(lib, rnn, **kw):
    from embodied_clip_amd import _lib
    h = C.c_void_p()
    return lib.ec_policy_create_rnn(C.byref(h), C.byref(_lib.PolicyCfg(**dict(REFERENCE, **kw))), rnn), h


def _layout(lib, h, shapes):
    offs = []
    for i in range(lib.ec_policy_num_param_tensors(h)):
        off, num = C.c_size_t(), C.c_size_t()
        assert lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)) == 0
        offs.append([off.value, num.value])
    return dict(flat_size=lib.ec_policy_flat_size(h), param_offsets=offs,
                workspace_bytes=[[T, N, b, lib.ec_policy_workspace_bytes(h, T, N, b)] for T, N in shapes for b in (0, 1)])


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    text = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert re.search(r"EC_RNN_GRU\s*=\s*0\s*,\s*EC_RNN_LSTM\s*=\s*1", header)
    assert _lib.RNN_TYPES == {"GRU": GRU, "LSTM": LSTM}
    # no field was added to the configuration struct: the cell is an argument of the new constructor
    assert [f[0] for f in _lib.PolicyCfg._fields_][-2:] == ["prev_action_dims", "prev_action_null"]
    # the header says what [N,H] is on an LSTM handle
    assert "[N,2H]" in text and "ec_policy_state_width" in text


def test_create_rnn_gru_is_todays_handle(lib, repo_root):
    """EC_RNN_GRU through the new constructor: the golden layout of tests/golden/policy_layout_golden.json, tensor for tensor and
    workspace for workspace."""
    golden = json.load(open(os.path.join(repo_root, "tests", "golden", "policy_layout_golden.json")))
    for name in ("reference", "small", "small7"):
        g = golden[name]
        shapes = sorted({(T, N) for T, N, _, _ in g["workspace_bytes"]}, key=[(T, N) for T, N, _, _ in g["workspace_bytes"]].index)
        rc, h = _create(lib, GRU, **g["cfg"])
        assert rc == 0
        try:
            got = _layout(lib, h, shapes)
            assert got["flat_size"] == g["flat_size"] and got["param_offsets"] == g["param_offsets"], name
            assert got["workspace_bytes"] == g["workspace_bytes"], name
            assert lib.ec_policy_rnn_type(h) == GRU and lib.ec_policy_state_width(h) == g["cfg"]["hidden"]
        finally:
            lib.ec_policy_destroy(h)
    # ... and ec_policy_create makes the same handle
    from embodied_clip_amd import _lib
    h = C.c_void_p()
    assert lib.ec_policy_create(C.byref(h), C.byref(_lib.PolicyCfg(**REFERENCE))) == 0
    assert lib.ec_policy_rnn_type(h) == GRU and lib.ec_policy_state_width(h) == 512
    lib.ec_policy_destroy(h)
    assert lib.ec_policy_rnn_type(None) == -1 and lib.ec_policy_state_width(None) == 0


@pytest.mark.parametrize("kw", [{}, dict(goal_in=3, num_actions=4), dict(prev_action_dims=6, prev_action_null=1),
                                dict(hidden=64, in_channels=64, num_actions=84, prev_action_dims=32)])
def test_lstm_layout(kw):
    from embodied_clip_amd.policy import PolicyHandle
    g, l = PolicyHandle(**kw), PolicyHandle(rnn_type="LSTM", **kw)
    H, E = l.H, l.prev_action_dims
    flat = 32 * 49
    assert list(l.offsets) == list(g.offsets) and l.param_order == g.param_order       # the same names in the same order
    assert l.shapes[RNN[0]] == (4 * H, flat + E) and l.shapes[RNN[1]] == (4 * H, H) and l.shapes[RNN[2]] == l.shapes[RNN[3]] == (4 * H,)
    for n in l.offsets:
        if n not in RNN:
            assert l.shapes[n] == g.shapes[n] and l.offsets[n][1] == g.offsets[n][1], n
        assert l.offsets[n][0] % 4 == 0
    grow = H * (flat + E) + H * H + 2 * H
    assert grow <= l.flat_size - g.flat_size < grow + 8                 # (each tensor starts 16-byte aligned)
    assert l.state_width == 2 * H and g.state_width == H and l.rnn_type == "LSTM"
    for (T, N) in ((1, 1), (1, 32), (8, 5), (128, 32)):
        for mode in (False, True):
            assert l.workspace_bytes(T, N, mode) >= g.workspace_bytes(T, N, mode), (T, N, mode)
        # at least the cell-state history and the fourth gate of the learn pass
        assert l.workspace_bytes(T, N, True) - g.workspace_bytes(T, N, True) >= 4 * T * N * H


def test_refusals(lib):
    assert _create(lib, LSTM, dual=1)[0] == -6                       # EC_ERR_UNSUPPORTED: the two-tower agent keeps the GRU
    assert _create(lib, LSTM, fusion=1, spatial=1)[0] == -6          # ... and the zero-shot agent
    assert _create(lib, 2)[0] == -1 and _create(lib, -1)[0] == -1    # EC_ERR_ARG
    assert _create(lib, LSTM, hidden=40)[0] == -2                    # hidden % 32
    assert _create(lib, GRU, hidden=40)[0] == 0                      # (the GRU handle takes it, as before)
    assert _create(lib, LSTM, hidden=640)[0] == -2                   # the forward step's tiles would not fit the LDS
    rc, h = _create(lib, LSTM, hidden=768)
    assert rc == 0 and lib.ec_policy_state_width(h) == 1536 and lib.ec_policy_rnn_type(h) == LSTM
    lib.ec_policy_destroy(h)
    from embodied_clip_amd.policy import PolicyHandle
    with pytest.raises(ValueError):
        PolicyHandle(rnn_type="RNN")


def test_step_argument_checks(lib):
    def fwd(a=P, whh=P, bhh=P, st=P, ld=128, mask=P, h=P, ldh=64, c=P, ldc=64, N=4, H=64):
        return lib.ec_lstm_step_fwd(a, whh, bhh, st, ld, mask, h, ldh, c, ldc, None, N, H, None)
    for k in ("a", "whh", "bhh", "st", "mask", "h", "c"):
        assert fwd(**{k: None}) == -1, k
    for kw in (dict(N=0), dict(H=40), dict(H=0), dict(ld=68), dict(ld=130, H=64), dict(ldh=32), dict(ldc=60), dict(H=640, ld=1280)):
        assert fwd(**kw) == -2, kw
    assert fwd(a=P + 4) == -1                                         # 16-byte alignment of the LDS-DMA operands

    def bwd(dhs=P, gates=P, c=P, cp=P, mask=P, whh=P, whhT=None, da_next=None, mask_next=None, ch=P, cc=P, da=P, N=4, H=256):
        return lib.ec_lstm_step_bwd(dhs, gates, c, cp, mask, whh, whhT, da_next, mask_next, ch, cc, da, N, H, None)
    for k in ("dhs", "gates", "c", "cp", "mask", "whh", "ch", "cc", "da"):
        assert bwd(**{k: None}) == -1, k
    assert bwd(whhT=P) == -1 and bwd(whhT=P, da_next=P) == -1         # the fused step needs step t+1's da and mask
    assert bwd(whhT=P, da_next=P, mask_next=P, H=64) == -2            # ... and H % 256 == 0
    assert bwd(N=0) == -2 and bwd(H=40) == -2


def test_synthetic_state_dict_shapes():
    from embodied_clip_amd import synthetic as syn
    sd = syn.policy_state_dict(0, hidden=64, in_channels=64, rnn_type="LSTM")
    g = syn.policy_state_dict(0, hidden=64, in_channels=64)
    assert list(sd) == list(g) and tuple(sd[RNN[0]].shape) == (256, 1568) and tuple(sd[RNN[1]].shape) == (256, 64)
    assert not sd[RNN[2]].any() and not sd[RNN[3]].any() and float(sd[RNN[1]].std()) > 0
    with pytest.raises(AssertionError):
        syn.policy_param_shapes(dual=1, rnn_type="LSTM")
