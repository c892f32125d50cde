"""The bounds tests/test_gpu_learn_routes.py holds the learn pass to (tests/_learn_route_ref.py) bite, checked without a GPU on
the cases of tests/_learn_route_cases.py with at most 5,000 rows:

  * the fp32 ORACLE against the float64 oracle stays under every exact-mode bound, whole tensor and worst row -- the condition
    that makes the bound legitimate: an fp32 evaluation in another summation order passes;
  * each named wrong version of the reference -- what a subtly wrong backward kernel would compute, built by perturbing the
    input of one oracle op (same values, one gradient path cut or re-routed), never by editing a kernel -- exceeds some bound
    by at least 4 x, on h256_t3_n33 (H = 256, T = 3, N = 33: 4,851 rows, a ragged second actor tile, a dh_final tensor;
    carry_no_reset on h32_t3_n5, whose last actor's mask column is 1, 1, 0 -- at step 1 the two mask rows differ):
      carry_no_reset        the last actor's recurrent gradient carry is scaled by step t + 1's mask row at step t
      dh_final_ignored      the backward never reads dh_final
      tile_rows_dropped     the 19 pixel rows of the last, partial 32-row tile add nothing to the encoder's weight gradients
      goal_neighbour        frame 1's goal-row gradient is credited to the neighbouring goal id
      wih_columns_swapped   weight_ih's gradient with two pixel columns swapped
      ragged_actor_bias     the ragged actor tile's last actor is dropped from the GRU's bias gradients;
  * the forward these wrong versions are hooked into is, without a hook, the oracle's own to the bit, gradients included."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _learn_route_ref as ref  # noqa: E402

cases = ref.cases
SMALL = [n for n in cases.DEFAULT_CASES if cases.rows_of(cases.CASES[n]) <= 5000]
WRONG_CASE = "h256_t3_n33"
WRONG_CASES = dict({w: WRONG_CASE for w in ref.WRONG}, carry_no_reset="h32_t3_n5")
_cache = {}


def _reference(name):
    """(state dict, inputs, float64 outputs, float64 gradients) of a case: computed once, shared, never changed"""
    if name not in _cache:
        case = cases.CASES[name]
        sd = ref.state_dict(case)
        inp = ref.make_inputs(case, sd)
        _cache[name] = (sd, inp, *ref.oracle(case, sd, inp))
    return _cache[name]


def test_small_cases_cover_the_table():
    assert len(SMALL) == len(cases.DEFAULT_CASES) - 2 and set(cases.DEFAULT_CASES) - set(SMALL) == {"pp_c128", "pp_c256"}
    assert set(ref.WRONG) == {"carry_no_reset", "dh_final_ignored", "tile_rows_dropped", "goal_neighbour", "wih_columns_swapped",
                              "ragged_actor_bias"}


def test_every_tensor_of_every_case_has_a_bound():
    for name in cases.DEFAULT_CASES:
        case = cases.CASES[name]
        for k in list(ref.state_dict(case)) + list(ref.OUTPUTS):
            assert 1e-7 < ref.FP32_ORACLE_ROW[k] < 2e-5, (name, k)      # 2^-24-class: nothing in the table is looser than 1.6e-4
    assert ref.EXACT_FACTOR == 8


@pytest.mark.parametrize("name", SMALL)
def test_fp32_oracle_meets_the_exact_bounds(name):
    case = cases.CASES[name]
    sd, inp, ro, rg = _reference(name)
    figs = ref.all_figures(*ref.oracle(case, sd, inp, torch.float32), ro, rg)
    for setting in ("exact", "default"):
        assert ref.violations(figs, setting) == [], name


def test_inputs_keep_every_relu_off_its_kink():
    """the conditioning of make_inputs(): no pre-activation within RELU_MARGIN of its layer's RMS; same draw every time"""
    case = cases.CASES[WRONG_CASE]
    sd, inp, _, _ = _reference(WRONG_CASE)
    cfg = cases.cfg_of(case)
    emb = sd[ref.GP + "embed_class.weight"].double()[inp["goal"].reshape(-1)]
    zs = ref._relu_inputs(cfg, sd, inp["feat"], emb, "")
    for z in zs:
        assert z.abs().min() >= 0.5 * ref.RELU_MARGIN * z.pow(2).mean().sqrt()      # (0.5: the RMS moves a little with the re-draws)
    again = ref.make_inputs(case, sd)
    assert all(torch.equal(again[k], inp[k]) for k in ("feat", "goal", "h0", "masks", "dhv", "dh_final"))


@pytest.mark.parametrize("name", [WRONG_CASE, "vec_t2_n21"])
def test_composed_forward_is_the_oracle(name):
    case = cases.CASES[name]
    sd, inp, ro, rg = _reference(name)
    co, cg = ref.oracle(case, sd, inp, composed=True)
    assert all(torch.equal(co[k], ro[k]) for k in ro) and all(torch.equal(cg[k], rg[k]) for k in rg)


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_wrong_version_exceeds_a_bound_fourfold(wrong):
    name = WRONG_CASES[wrong]
    case = cases.CASES[name]
    sd, inp, ro, rg = _reference(name)
    T, N = case["T"], case["N"]
    if name == WRONG_CASE:
        assert case["dhf"] and N % 32 == 1 and cases.rows_of(case) % 32 == 19
    else:       # (the state entering step 0 is an input: only a step t >= 1 carries a gradient back)
        assert inp["masks"][:, N - 1].tolist() == [1.0, 1.0, 0.0]
    wo, wg = ref.oracle(case, sd, inp, wrong=wrong)
    # a wrong version changes gradients only (ragged_actor_bias adds the biases in an op of its own: float64 rounding)
    assert all(ref.rel_l2(wo[k], ro[k]) < 1e-13 if wrong == "ragged_actor_bias" else torch.equal(wo[k], ro[k]) for k in ro)
    figs = ref.all_figures(wo, wg, ro, rg)
    over = {k: max(rel, row) / ref.bound(k) for k, (rel, row) in figs.items()}
    worst = max(over, key=over.get)
    print("%s: %s at %.1f x its bound (rel-L2 %.2e, worst row %.2e)" % (wrong, worst, over[worst], *figs[worst]))
    assert over[worst] >= 4, (wrong, worst, over[worst])
    assert any(k == worst and what == "row" for k, what, _, _ in ref.violations(figs, "exact"))
