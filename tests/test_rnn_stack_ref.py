"""The multi-layer reference of tests/_rnn_stack_ref.py on the CPU: it IS torch.nn.GRU / torch.nn.LSTM(num_layers=L) between mask
zeros; the memory conversions; the fp32 reference keeps a tenth of every bound the GPU tests use; deliberately wrong variants
miss their bound by a wide margin (the factor is printed)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rnn_stack_ref as ref  # noqa: E402

GRU, LSTM = ref.GRU, ref.LSTM


def _torch_rnn(cell, I, H, L, seed):
    torch.manual_seed(seed)
    rnn = (torch.nn.GRU if cell == GRU else torch.nn.LSTM)(I, H, num_layers=L).double()
    sd = {f"state_encoder.rnn.{k}": v.detach() for k, v in rnn.state_dict().items()}
    return rnn, sd


@pytest.mark.parametrize("cell", [GRU, LSTM])
@pytest.mark.parametrize("L", [2, 3])
def test_stack_is_torch_rnn_segment_by_segment(cell, L):
    """Between mask zeros the stack equals torch's module run on the segment from the carried memory; at a zero the module
    restarts from a memory whose masked actors are zeroed in EVERY layer (h and c)."""
    T, N, I, H = 7, 4, 12, 8
    rnn, sd = _torch_rnn(cell, I, H, L, 3 + L)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, N, I, generator=g, dtype=torch.float64)
    k = 2 if cell == LSTM else 1
    mem = torch.randn(k * L, N, H, generator=g, dtype=torch.float64)
    masks = torch.ones(T, N, 1, dtype=torch.float64)
    masks[0, 1] = 0
    masks[3, 0] = 0
    masks[3, 2] = 0
    masks[5, 3] = 0
    state0 = ref.memory_to_state(mem, cell, L)
    out, state = ref.sequence(cell, x, state0, masks, sd)

    def run(seg, mem):
        """torch's module over x[seg] in ONE call from `mem` -> (outputs, new memory)"""
        if cell == LSTM:
            o, (h, c) = rnn(x[seg], (mem[:L].contiguous(), mem[L:].contiguous()))
            return o, torch.cat([h, c], 0)
        return rnn(x[seg], mem.contiguous())

    # segments between the steps that hold a mask zero: 0 | 1..2 | 3..4 | 5..6; the memory of every layer (h and c) is masked
    # in front of each segment, which is what RNNStateEncoder does at a reset
    outs = []
    with torch.no_grad():
        for seg in (slice(0, 1), slice(1, 3), slice(3, 5), slice(5, 7)):
            mem = mem * masks[seg.start].view(1, N, 1)
            o, mem = run(seg, mem)
            outs.append(o)
    want = torch.cat(outs, 0)
    assert (out - want).abs().max() < 1e-12
    assert (ref.state_to_memory(state, cell, L) - mem).abs().max() < 1e-12


@pytest.mark.parametrize("cell", [GRU, LSTM])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_memory_conversions(cell, L):
    from embodied_clip_amd import policy
    N, H = 3, 4
    k = 2 if cell == LSTM else 1
    h = torch.arange(L * N * H, dtype=torch.float32).view(L, N, H)
    c = -h - 1
    mem = torch.cat([h, c], 0) if cell == LSTM else h
    for to_state, to_mem in ((ref.memory_to_state, ref.state_to_memory), (policy.memory_to_state, policy.state_to_memory)):
        st = to_state(mem, cell, L)
        assert tuple(st.shape) == (N, L * k * H)
        for l in range(L):
            assert torch.equal(st[:, l * k * H:l * k * H + H], h[l])                      # layer l's slice starts with its h ...
            if cell == LSTM:
                assert torch.equal(st[:, l * k * H + H:(l + 1) * k * H], c[l])            # ... followed by its c
        assert torch.equal(to_mem(st, cell, L), mem)
    with pytest.raises(ValueError):
        policy.memory_to_state(mem[:-1] if mem.shape[0] > 1 else mem.repeat(2, 1, 1), cell, L)
    with pytest.raises(ValueError):
        policy.state_to_memory(torch.zeros(N, 2, L * k * H), cell, L)


def test_fp32_reference_keeps_a_tenth_of_every_bound():
    for k, (v, case) in ref.kernel_fp32_distance().items():
        print(f"kernel {k}: fp32-vs-float64 rel-L2 {v:.3e} at {case}; GPU bound {10 * v:.3e}")
        assert v <= 0.1 * ref.kernel_bounds()[k] * (1 + 1e-12) and v < 1e-6
    for case in ref.POLICY_CASES:
        fwd, grad = ref.policy_fp32_distance(case)
        print(f"policy {case}: fp32-vs-float64 forward {fwd:.3e} (bound {ref.FWD_TOL:.0e}), worst gradient {grad:.3e} (bound {ref.GRAD_TOL:.0e})")
        assert fwd <= 0.1 * ref.FWD_TOL and grad <= 0.1 * ref.GRAD_TOL, case


def test_masks_have_zeros_at_the_start_and_in_the_middle():
    for case in ref.POLICY_CASES:
        T = case[0]
        m = ref.policy_inputs(*case)[2]["masks"]
        assert (m[0] == 0).any() and (m[0] == 1).any() or case[1] == 1
        if T > 2:
            assert (m[T // 2] == 0).any()


WRONG = [("mask_x", ref.POLICY_CASES[0]), ("mask_x", ref.POLICY_CASES[1]), ("skip_layer", ref.POLICY_CASES[1]),
         ("xn_inside", ref.POLICY_CASES[0]), ("swap_hc", ref.POLICY_CASES[1]), ("drop_bih", ref.POLICY_CASES[0]),
         ("drop_bih", ref.POLICY_CASES[1])]


@pytest.mark.parametrize("wrong,case", WRONG)
def test_wrong_variants_miss_the_forward_bound(wrong, case):
    """the mask also applied to x | layer 2 fed layer 0's output | the GRU's x_n inside r * (...) | h and c swapped in the state
    row | the upper layer's b_ih dropped: each at least 100 x the forward bound away from the reference"""
    cell, null = case[10], case[6]
    cfg, sd, b = ref.policy_inputs(*case)
    sd64 = {k: v.double() for k, v in sd.items()}
    args = (b["feat"].double(), b["goal"].double() if b["goal"].is_floating_point() else b["goal"], b["prev_actions"], b["h0"].double(),
            b["masks"].double(), sd64, null)
    with torch.no_grad():
        good = ref.actor_critic_forward(cell, *args)
        bad = ref.actor_critic_forward(cell, *args, wrong=wrong)
    e = max(ref.rel_l2(bad[0], good[0]), ref.rel_l2(bad[2], good[2]))
    print(f"{wrong} at {case}: rel-L2 {e:.3e} = {e / ref.FWD_TOL:.0f} x the forward bound")
    assert e > 100 * ref.FWD_TOL, (wrong, e)


@pytest.mark.parametrize("cell", [GRU, LSTM])
def test_wrong_variants_miss_the_kernel_bound(cell):
    """one layer's step alone: the mask on x, and the dropped b_ih, against the kernel bound"""
    N, H = 33, 64
    d = ref.kernel_inputs(cell, N, H)
    m = ref.kernel_mask(N, "mixed")
    good = ref.kernel_reference(cell, d, m)
    bound = ref.kernel_bounds()[(cell, "h")]
    masked_x = ref.kernel_reference(cell, dict(d, x=d["x"] * m.view(-1, 1)), m)
    no_bih = ref.kernel_reference(cell, dict(d, bih=torch.zeros_like(d["bih"])), m)
    for name, bad in (("mask on x", masked_x), ("b_ih dropped", no_bih)):
        e = ref.rel_l2(bad[:, :H], good[:, :H])
        print(f"{cell} {name}: rel-L2 {e:.3e} = {e / bound:.0f} x the kernel bound")
        assert e > 100 * bound
