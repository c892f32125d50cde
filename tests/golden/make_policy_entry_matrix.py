"""Records the return code of every policy forward, act and backward entry point for a cross of handles and argument patterns
(CPU only: every row passes ws_bytes = 0, so a call the entry point accepts ends in EC_ERR_WORKSPACE in front of its first HIP
call, and no pointer is read), and every handle's flat tensor table as ec_policy_param_offset reports it:

    EC_AMD_LIB=/path/to/libec_amd.so python tests/golden/make_policy_entry_matrix.py      (from the repository root)

  tests/golden/policy_entry_matrix.json   `codes`: entry point -> handle -> one return code per pattern of patterns(entry);
                                          `layout`: handle -> tensor count, flat size, [offset, elements] per tensor, and the
                                          codes of the out-of-range lookups

The committed table was written by the library of commit 2f47d9e, the last one whose entry points checked their arguments
inline; tests/test_policy_entry_matrix.py holds every later build to it.  The odd rows are pinned as they are, not judged: a
NULL handle is EC_ERR_UNSUPPORTED from ec_policy_act but EC_ERR_ARG from ec_policy_act_ex, and
ec_policy_num_param_tensors(NULL) is not 0."""
import ctypes as C
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "policy_entry_matrix.json")
PARENT_COMMIT = "2f47d9e"
OK, ARG, SHAPE, LAUNCH, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -4, -6

# ---- the entry points: their arguments by name, in order ------------------------------------------------------------------
_FWD_TAIL = "h0 masks T N workspace ws_bytes mode hv h_final stream"
_ACT_TAIL = "h0 masks N workspace ws_bytes reuse hv h_final actions logp values"
_SEL = "greedy seed step first_actor expert mask force_p stream"
_BWD_TAIL = "masks T N workspace ws_bytes dhv dh_final grads"
ENTRIES = {k: v.split() for k, v in {
    "ec_policy_forward": "h params feat bf16 goal " + _FWD_TAIL,
    "ec_policy_forward2": "h params feat feat2 bf16 goal " + _FWD_TAIL,
    "ec_policy_forward_vec": "h params feat feat2 bf16 goal_vec " + _FWD_TAIL,
    "ec_policy_forward_pa": "h params feat feat2 bf16 goal goal_vec prev " + _FWD_TAIL,
    "ec_policy_forward_pooled": "h params feat goal sensors prev " + _FWD_TAIL,
    "ec_policy_forward_two_view": "h params feat feat2 prev " + _FWD_TAIL,
    "ec_policy_act": "h params feat feat2 bf16 goal " + _ACT_TAIL + " seed step first_actor stream",
    "ec_policy_act_vec": "h params feat feat2 bf16 goal_vec " + _ACT_TAIL + " seed step first_actor stream",
    "ec_policy_act_greedy": "h params feat feat2 bf16 goal " + _ACT_TAIL + " stream",
    "ec_policy_act_vec_greedy": "h params feat feat2 bf16 goal_vec " + _ACT_TAIL + " stream",
    "ec_policy_act_ex": "h params feat feat2 bf16 goal goal_vec " + _ACT_TAIL + " " + _SEL,
    "ec_policy_act_pa": "h params feat feat2 bf16 goal goal_vec prev " + _ACT_TAIL + " " + _SEL,
    "ec_policy_act_pooled": "h params feat goal sensors prev " + _ACT_TAIL + " " + _SEL,
    "ec_policy_act_two_view": "h params feat feat2 prev " + _ACT_TAIL + " " + _SEL,
    "ec_policy_backward": "h params feat bf16 " + _BWD_TAIL + " stream",
    "ec_policy_backward2": "h params feat feat2 bf16 " + _BWD_TAIL + " stream",
    "ec_policy_backward3": "h params feat feat2 bf16 " + _BWD_TAIL + " event stream",
}.items()}
INTS = {"bf16", "T", "N", "ws_bytes", "mode", "reuse", "greedy", "seed", "step", "first_actor", "force_p"}
NEVER_FLIPPED = {"h", "stream", "event"}

# ---- the handles ----------------------------------------------------------------------------------------------------------
_SMALL = dict(in_channels=64, spatial=7, hidden=64, goal_dims=32, num_goals=12, num_actions=6, compress_hid=128, compress_out=32,
              comb_hid=128, comb_out=32)
HANDLES = {
    "null": None,
    "ids": ("tensor", dict(_SMALL), 0, 1),
    "vec2": ("tensor", dict(_SMALL, goal_in=2), 0, 1),
    "dual": ("tensor", dict(_SMALL, dual=1), 0, 1),
    "fusion": ("tensor", dict(_SMALL, fusion=1, spatial=1), 0, 1),
    "pa8": ("tensor", dict(_SMALL, prev_action_dims=8, prev_action_null=1), 0, 1),
    "wide20": ("tensor", dict(_SMALL, num_actions=20), 0, 1),
    "lstm2": ("tensor", dict(_SMALL), 1, 2),
    "pooled_full": ("pooled", dict(embed_in=64, hidden=64, embed_dims=32, num_goals=12, num_sensors=2, sensor_in=(2, 2, 0), num_actions=6,
                                   prev_action_dims=8, prev_action_null=1, rnn_type=0, num_layers=1)),
    "pooled_sensor": ("pooled", dict(embed_in=64, hidden=64, embed_dims=32, num_goals=0, num_sensors=1, sensor_in=(3, 0, 0), num_actions=6,
                                     prev_action_dims=0, prev_action_null=0, rnn_type=0, num_layers=1)),
    "two_view_pa": ("two_view", dict(in_channels=64, spatial=2, hidden=64, attn_hidden=32, num_actions=20, prev_action_dims=8,
                                     prev_action_null=1, rnn_type=1, num_layers=1)),
    "two_view": ("two_view", dict(in_channels=64, spatial=2, hidden=64, attn_hidden=32, num_actions=20, prev_action_dims=0,
                                  prev_action_null=0, rnn_type=1, num_layers=2)),
}


def create(lib, _lib, name):
    spec = HANDLES[name]
    if spec is None:
        return None
    h = C.c_void_p()
    if spec[0] == "tensor":
        rc = lib.ec_policy_create_rnn_layers(C.byref(h), C.byref(_lib.PolicyCfg(**spec[1])), spec[2], spec[3])
    elif spec[0] == "pooled":
        rc = lib.ec_policy_create_pooled(C.byref(h), C.byref(_lib.PooledCfg(**dict(spec[1], sensor_in=(C.c_int * 3)(*spec[1]["sensor_in"])))))
    else:
        rc = lib.ec_policy_create_two_view(C.byref(h), C.byref(_lib.TwoViewCfg(**spec[1])))
    assert rc == OK and h.value, (name, rc)
    return h


def _ptr(name, names):
    """a distinct, 256-byte aligned fake address per argument name; never read"""
    return 0x10000000 + 0x1000 * (sorted(names).index(name) + 1)


def valid_args(entry, handle):
    """the all-valid arguments of `entry` for the face `handle` belongs to (for the null handle: the plain id handle's)"""
    spec = HANDLES[handle] or HANDLES["ids"]
    kind, cfg = spec[0], spec[1]
    names = ENTRIES[entry]
    a = {n: _ptr(n, names) for n in names if n not in INTS}
    a.update(h=None, stream=0, event=0, bf16=0 if kind == "pooled" else 1, T=2, N=4, ws_bytes=0, mode=0, reuse=0, greedy=0, seed=1, step=2,
             first_actor=0, force_p=0.0, expert=0, mask=0, dh_final=0)
    a["feat2"] = a.get("feat2", 0) if kind == "two_view" or cfg.get("dual") else 0
    a["goal"] = a.get("goal", 0) if (kind == "tensor" and not cfg.get("goal_in")) or (kind == "pooled" and cfg["num_goals"]) else 0
    a["goal_vec"] = a.get("goal_vec", 0) if kind == "tensor" and cfg.get("goal_in") else 0
    a["prev"] = a.get("prev", 0) if cfg.get("prev_action_dims") else 0
    a["sensors"] = a.get("sensors", 0) if kind == "pooled" and cfg["num_sensors"] else 0
    return {n: a[n] for n in names}


# a pattern: name -> function(arguments, entry's names) that edits the arguments; a pattern that names an argument the entry
# point does not have is left out of patterns(entry)
def _set(**kw):
    return lambda a, names: a.update({k: (_ptr(k, names) if v == "ptr" else v) for k, v in kw.items()})


def _flip(n):
    return lambda a, names: a.update({n: 0 if a[n] else _ptr(n, names)})


def _swap(a, names):
    a["goal"], a["goal_vec"] = a["goal_vec"], a["goal"]


FIXED = [
    ("valid", (), lambda a, names: None),
    ("goal_swapped", ("goal", "goal_vec"), _swap),
    ("goal_both", ("goal", "goal_vec"), _set(goal="ptr", goal_vec="ptr")),
    ("feat_off_4", ("feat",), lambda a, names: a.update(feat=a["feat"] + 4)),
    ("feat2_off_4", ("feat2",), lambda a, names: a.update(feat2=_ptr("feat2", names) + 4)),
    ("T0", ("T",), _set(T=0)),
    ("N0", ("N",), _set(N=0)),
    ("N_negative", ("N",), _set(N=-3)),
    ("mode3", ("mode",), _set(mode=3)),
    ("mode_learn", ("mode",), _set(mode=1)),
    ("mode_reuse", ("mode",), _set(mode=2)),
    ("reuse1", ("reuse",), _set(reuse=1)),
    ("bf16_0", ("bf16",), _set(bf16=0)),
    ("h_final_is_h0", ("h_final", "h0"), lambda a, names: a.update(h_final=a["h0"])),
    ("first_actor_m1", ("first_actor",), _set(first_actor=-1)),
    ("greedy", ("greedy",), _set(greedy=1)),
    ("greedy_first_actor_m1", ("greedy",), _set(greedy=1, first_actor=-1)),
    ("forcing", ("expert",), _set(expert="ptr", mask="ptr", force_p=0.5)),
    ("forcing_p0", ("expert",), _set(expert="ptr", mask="ptr")),
    ("forcing_p1", ("expert",), _set(expert="ptr", mask="ptr", force_p=1.0)),
    ("force_p_1.5", ("expert",), _set(expert="ptr", mask="ptr", force_p=1.5)),
    ("force_p_nan", ("expert",), _set(expert="ptr", mask="ptr", force_p=math.nan)),
    ("force_p_negative", ("expert",), _set(expert="ptr", mask="ptr", force_p=-0.25)),
    ("force_p_without_expert", ("expert",), _set(force_p=0.5)),
    ("force_p_1.5_without_expert", ("expert",), _set(force_p=1.5)),
    ("force_p_nan_without_expert", ("expert",), _set(force_p=math.nan)),
    ("expert_without_mask", ("expert",), _set(expert="ptr", force_p=0.5)),
    ("mask_without_expert", ("expert",), _set(mask="ptr", force_p=0.5)),
    ("greedy_with_expert", ("expert",), _set(greedy=1, expert="ptr", mask="ptr", force_p=0.5)),
    # two faults at once: which code wins
    ("T0+N0", ("T",), _set(T=0, N=0)),
    ("T0+mode3", ("T", "mode"), _set(T=0, mode=3)),
    ("N0+mode3", ("mode",), _set(N=0, mode=3)),
    ("N0+no_params", ("N",), _set(N=0, params=0)),
    ("N0+no_hv", ("N", "hv"), _set(N=0, hv=0)),
    ("N0+feat_off_4", ("N",), lambda a, names: a.update(N=0, feat=a["feat"] + 4)),
    ("mode3+no_masks", ("mode",), _set(mode=3, masks=0)),
    ("no_actions+N0", ("actions",), _set(actions=0, N=0)),
    ("no_logp+no_params", ("logp",), _set(logp=0, params=0)),
    ("first_actor_m1+no_params", ("first_actor",), _set(first_actor=-1, params=0)),
    ("first_actor_m1+N0", ("first_actor",), _set(first_actor=-1, N=0)),
    ("first_actor_m1+no_actions", ("first_actor",), _set(first_actor=-1, actions=0)),
    ("first_actor_m1+expert_without_mask", ("expert",), _set(first_actor=-1, expert="ptr")),
    ("first_actor_m1+force_p_nan", ("expert",), _set(first_actor=-1, expert="ptr", mask="ptr", force_p=math.nan)),
    ("greedy_with_expert+N0", ("expert",), _set(greedy=1, expert="ptr", mask="ptr", N=0)),
    ("forcing+no_feat", ("expert",), _set(expert="ptr", mask="ptr", force_p=0.5, feat=0)),
    ("no_dhv+T0", ("dhv",), _set(dhv=0, T=0)),
]


def patterns(entry):
    """[(name, edit)] for `entry`: the fixed patterns its arguments admit, then every pointer flipped (NULL where the valid call
    has one, a pointer where it has NULL) in turn"""
    names = ENTRIES[entry]
    out = [(n, f) for n, need, f in FIXED if all(k in names for k in need)]
    out += [("flip_" + n, _flip(n)) for n in names if n not in INTS and n not in NEVER_FLIPPED]
    return out


def call(lib, entry, h, args):
    vals = [h if n == "h" else args[n] for n in ENTRIES[entry]]
    return int(getattr(lib, entry)(*vals))


def record(lib, _lib):
    """-> dict(codes=..., layout=...) of the loaded library"""
    handles = {n: create(lib, _lib, n) for n in HANDLES}
    codes, layout = {}, {}
    for entry, names in ENTRIES.items():
        codes[entry] = {}
        for hn, h in handles.items():
            row = []
            for _pn, edit in patterns(entry):
                a = valid_args(entry, hn)
                edit(a, names)
                row.append(call(lib, entry, h, a))
            codes[entry][hn] = row
    for hn, h in handles.items():
        n = lib.ec_policy_num_param_tensors(h)
        off, num = C.c_size_t(), C.c_size_t()
        table = []
        for i in range(n if h is not None else 0):
            assert lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)) == OK, (hn, i)
            table.append([off.value, num.value])
        edges = [lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)) for i in (-1, n, n + 1, 1 << 20)]
        edges += [lib.ec_policy_param_offset(h, 0, None, C.byref(num)), lib.ec_policy_param_offset(h, 0, C.byref(off), None)]
        layout[hn] = dict(count=n, flat=lib.ec_policy_flat_size(h), table=table, edges=edges,
                          ws=[lib.ec_policy_workspace_bytes(h, *a) for a in ((1, 4, 0), (2, 4, 1), (0, 4, 0), (2, 0, 1), (2, 4, 3))],
                          kind=[lib.ec_policy_is_pooled(h), lib.ec_policy_is_two_view(h), lib.ec_policy_rnn_type(h), lib.ec_policy_rnn_layers(h),
                                lib.ec_policy_state_width(h)])
    for h in handles.values():
        if h is not None:
            lib.ec_policy_destroy(h)
    return dict(codes=codes, layout=layout)


def matching(entry, handle):
    """is `handle` one that `entry` serves (its all-valid row has to come back EC_ERR_WORKSPACE)?"""
    spec = HANDLES[handle]
    if spec is None:
        return False
    kind, cfg = spec[0], spec[1]
    if "backward" in entry:
        return entry != "ec_policy_backward" or not (cfg.get("dual") or kind == "two_view")
    face = "pooled" if "pooled" in entry else "two_view" if "two_view" in entry else "tensor"
    if face != kind:
        return False
    if kind != "tensor":
        return True
    if bool(cfg.get("prev_action_dims")) != entry.endswith("_pa"):
        return False
    if entry in ("ec_policy_act_ex", "ec_policy_act_pa", "ec_policy_forward_pa"):
        return True
    if "act" in entry and cfg["num_actions"] > 7:
        return False
    if entry == "ec_policy_forward" and cfg.get("dual"):
        return False
    return ("_vec" in entry) == bool(cfg.get("goal_in"))


def check(table):
    """the conditions a recorded table has to meet"""
    for entry, by_handle in table["codes"].items():
        for hn, row in by_handle.items():
            assert len(row) == len(patterns(entry)), (entry, hn)
            assert OK not in row and LAUNCH not in row, (entry, hn, row)
            assert (row[0] == WORKSPACE) == matching(entry, hn), (entry, hn, row[0])
        assert any(matching(entry, hn) for hn in by_handle), entry


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from embodied_clip_amd import _lib  # noqa: E402
    table = dict(parent_commit=PARENT_COMMIT, **record(_lib.load(), _lib))
    check(table)
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(table, separators=(",", ":")).replace('],"', '],\n"').replace('},"', '},\n"'))
    rows = sum(len(r) for e in table["codes"].values() for r in e.values())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes from", _lib.LIB_PATH, "-", rows, "rows")
