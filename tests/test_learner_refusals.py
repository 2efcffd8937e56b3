"""One check, every call: the chain learners' C calls share one host front end
(dronerl_amd/csrc/dronerl_learn_front.h over dronerl_learn_args.h), so a bad
argument is refused with the same text by every family's call.

One table of faults is applied to all eleven train calls (uniform x {dense,
wide, conv, conv-large}, prioritized x {dense, wide, conv-large}, Double x
{dense, wide} x {uniform, prioritized}), and its parts to the four init,
sample_rows and layout_query calls.  The two deliberate differences are
named in the table.  No GPU: every call here has a fault and returns before
any device work (the device pointers are fake and never dereferenced); no
call with all arguments good is ever issued."""
import ctypes

import pytest

vp = ctypes.c_void_p
AGENT, PACKED, PER, SLOTS, RING = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24

# ---- the two differences between the calls, by name ------------------------
# 1. f32 rows shorter than the net's input: the conv nets name their input by its window
SHORT_ROWS = {"dense": "replay obs_floats < in_features", "wide": "replay obs_floats < in_features",
              "conv": "replay obs_floats < window * window * 6"}
# 2. a ring too large (or empty): the prioritized calls take the refusal from the tree's plan (per::plan), whose
#    limit is lower
CAPACITY = {False: "replay capacity must be in [1, 2^31)", True: "capacity must be in [1, 2^24] (DRL_PER_MAX_CAPACITY)"}

AGENT_TEXT = "the agent block must be a 16-byte aligned device pointer"
PACKED_TEXT = "packed buffer must be a 16-byte aligned device pointer"
PER_TEXT = "the prioritized replay block must be a 16-byte aligned device pointer"
RING_NULL = "replay buffers are NULL"
SIZE_TEXT = "size must be in [0, capacity]"

# fault -> (the refusal's whole text, or a function of (family, prioritized); the mutation of the good call).
# "per" faults are the prioritized calls' alone.
TRAIN_FAULTS = {
    "h NULL": ("hparams is NULL", lambda s: s.update(h=None)),
    "target_update_interval 0": ("target_update_interval and epsilon_decay_every must be >= 1",
                                 lambda s: s["h"].update(target_update_interval=0)),
    "epsilon_decay_every 0": ("target_update_interval and epsilon_decay_every must be >= 1",
                              lambda s: s["h"].update(epsilon_decay_every=0)),
    "beta1 1.0": ("beta1 and beta2 must be in [0, 1)", lambda s: s["h"].update(beta1=1.0)),
    "beta2 -0.5": ("beta1 and beta2 must be in [0, 1)", lambda s: s["h"].update(beta2=-0.5)),
    "agent NULL": (AGENT_TEXT, lambda s: s.update(agent=None)),
    "agent misaligned": (AGENT_TEXT, lambda s: s.update(agent=AGENT + 8)),
    "packed NULL": (PACKED_TEXT, lambda s: s.update(packed=None)),
    "packed misaligned": (PACKED_TEXT, lambda s: s.update(packed=PACKED + 4)),
    "r NULL": (RING_NULL, lambda s: s.update(r=None)),
    "r.obs NULL": (RING_NULL, lambda s: s["r"].update(obs=None)),
    "r.next_obs NULL": (RING_NULL, lambda s: s["r"].update(next_obs=None)),
    "r.actions NULL": (RING_NULL, lambda s: s["r"].update(actions=None)),
    "r.rewards NULL": (RING_NULL, lambda s: s["r"].update(rewards=None)),
    "r.dones NULL": (RING_NULL, lambda s: s["r"].update(dones=None)),
    "capacity 0": (lambda fam, per: CAPACITY[per], lambda s: s["r"].update(capacity=0)),
    "capacity 2^31": (lambda fam, per: CAPACITY[per], lambda s: s["r"].update(capacity=1 << 31)),
    "size -1": (SIZE_TEXT, lambda s: s.update(size=-1)),
    "size capacity+1": (SIZE_TEXT, lambda s: s.update(size=s["r"]["capacity"] + 1)),
    "short rows": (lambda fam, per: SHORT_ROWS[fam], lambda s: s["r"].update(obs_floats=292)),
    "f32 rows for a code net": ("a DRL_QNET_INPUT_CODE net's replay rows are policy codes "
                                "(drl_policy_code_bytes / 4 words)", lambda s: s.update(desc="code")),
    "rows misaligned": ("replay rows must be 4-byte aligned", lambda s: s["r"].update(obs=RING + 2)),
    "next rows misaligned": ("replay rows must be 4-byte aligned", lambda s: s["r"].update(next_obs=RING + (1 << 20) + 1)),
    "per: ph NULL": ("the prioritized replay's hparams are NULL", lambda s: s.update(ph=None)),
    "per: alpha -1": ("alpha must be >= 0", lambda s: s["ph"].update(alpha=-1.0)),
    "per: beta0 2": ("beta0 must be in [0, 1]", lambda s: s["ph"].update(beta0=2.0)),
    "per: block NULL": (PER_TEXT, lambda s: s.update(per=None)),
    "per: block misaligned": (PER_TEXT, lambda s: s.update(per=PER + 8)),
}
# what the family's own plan refuses, in the plan's words: the text names the family's limit behind this prefix
PLAN_FAULTS = {
    "batch 0": ("batch must be in [1, ", lambda s: (s["h"].update(batch=0), s.update(batch=0))),
    "batch 4097": ("batch must be in [1, ", lambda s: (s["h"].update(batch=4097), s.update(batch=4097))),
    "a fourth hidden / conv layer": (" must be 1, 2 or 3", lambda s: s.update(desc="bad")),
}

# call -> (family, prioritized)
TRAIN_CALLS = {
    "drl_dqn_large_train": ("dense", False), "drl_widenet_dqn_train": ("wide", False),
    "drl_convnet_dqn_train": ("conv", False), "drl_convnet_dqn_large_train": ("conv", False),
    "drl_dqn_per_train": ("dense", True), "drl_widenet_dqn_per_train": ("wide", True),
    "drl_convnet_dqn_per_train": ("conv", True),
    "drl_dqn_double_train": ("dense", False), "drl_widenet_dqn_double_train": ("wide", False),
    "drl_dqn_double_per_train": ("dense", True), "drl_widenet_dqn_double_per_train": ("wide", True),
}
OTHER_CALLS = {"dense": "drl_dqn_large_", "wide": "drl_widenet_dqn_", "conv": "drl_convnet_dqn_",
               "conv-large": "drl_convnet_dqn_large_"}


@pytest.fixture(scope="module")
def L():
    from dronerl_amd import dqn
    from dronerl_amd._native import lib
    return dqn._bind_widenet(dqn._bind_convnet(dqn._bind(lib())))


def _desc(fam, kind):
    from dronerl_amd import dqn
    inp = 1 if kind == "code" else 0
    if fam == "dense":
        d = dqn.DrlQnetDesc(294, 2, (ctypes.c_int32 * 3)(128, 64, 0), 5, 1, inp)
    elif fam == "wide":
        d = dqn.DrlWidenetDesc(294, 2, (ctypes.c_int32 * 3)(256, 128, 0), 5, inp)
    else:
        d = dqn.convnet_desc((7, 7, 6), ({"out_channels": 4, "kernel_size": 3, "stride": 1, "padding": 1},), (8,), 5,
                             "code" if inp else "obs")
    if kind == "bad":
        setattr(d, "n_conv" if fam.startswith("conv") else "n_hidden", 4)
    return d


def _good():
    return dict(desc="good", h=dict(batch=32), ph=dict(alpha=0.6, beta0=0.4, beta_steps=1000, eps=1e-6),
                agent=AGENT, packed=PACKED, per=PER, slots=SLOTS, size=100, batch=32, layout=True,
                r=dict(capacity=5000, obs_floats=294, obs=RING, next_obs=RING + (1 << 20), actions=RING + (2 << 20),
                       rewards=RING + (3 << 20), dones=RING + (4 << 20)))


def _refusal(L, rc):
    assert rc != 0
    return L.drl_last_error().decode()


def _train(L, call, fam, per, s):
    from dronerl_amd import dqn
    d = _desc(fam, s["desc"])
    h = None if s["h"] is None else ctypes.byref(dqn.DQNHParams(**s["h"]).c())
    r = None if s["r"] is None else ctypes.byref(dqn.DrlReplay(*(s["r"][k] for k in (
        "capacity", "obs_floats", "obs", "next_obs", "actions", "rewards", "dones"))))
    f = getattr(L, call)
    if not per:
        return _refusal(L, f(ctypes.byref(d), h, vp(s["agent"]), vp(s["packed"]), r, s["size"], None))
    ph = None if s["ph"] is None else ctypes.byref(dqn.DrlPerHParams(*(s["ph"][k] for k in (
        "alpha", "beta0", "beta_steps", "eps"))))
    return _refusal(L, f(ctypes.byref(d), h, ph, vp(s["agent"]), vp(s["packed"]), r, s["size"], vp(s["per"]), None))


def _faulty(mutate):
    s = _good()
    mutate(s)
    assert s != _good()     # never a call with every argument good
    return s


def test_every_train_call_refuses_every_fault_with_the_one_text(L):
    assert len(TRAIN_CALLS) == 11
    for name, (text, mutate) in TRAIN_FAULTS.items():
        said = {}
        for call, (fam, per) in TRAIN_CALLS.items():
            if name.startswith("per: ") and not per:
                continue
            got = _train(L, call, fam, per, _faulty(mutate))
            assert got == (text(fam, per) if callable(text) else text), (call, name, got)
            said[call] = got
        if not callable(text):
            assert len(set(said.values())) == 1, (name, said)
    for name, (part, mutate) in PLAN_FAULTS.items():
        for call, (fam, per) in TRAIN_CALLS.items():
            got = _train(L, call, fam, per, _faulty(mutate))
            assert part in got, (call, name, got)


def _other(L, prefix, what, fam, s):
    from dronerl_amd import dqn
    d = _desc("conv" if fam.startswith("conv") else fam, s["desc"])
    f = getattr(L, prefix + what)
    if what == "init":
        return _refusal(L, f(ctypes.byref(d), s["batch"], vp(s["agent"]), 1.0, None))
    if what == "sample_rows":
        h = None if s["h"] is None else ctypes.byref(dqn.DQNHParams(**s["h"]).c())
        return _refusal(L, f(ctypes.byref(d), h, vp(s["agent"]), s["size"], vp(s["slots"]), None))
    lay = (dqn.DrlConvnetDqnLayout if fam.startswith("conv") else dqn.DrlDqnLayout)()
    return _refusal(L, f(ctypes.byref(d), s["batch"], ctypes.byref(lay) if s["layout"] else None))


SLOTS_TEXT = "d_slots must be an 8-byte aligned device pointer"
OTHER_FAULTS = {
    "init": {
        "agent NULL": (AGENT_TEXT, lambda s: s.update(agent=None)),
        "agent misaligned": (AGENT_TEXT, lambda s: s.update(agent=AGENT + 4)),
    },
    "sample_rows": {
        "h NULL": ("hparams is NULL", lambda s: s.update(h=None)),
        "agent NULL": (AGENT_TEXT, lambda s: s.update(agent=None)),
        "agent misaligned": (AGENT_TEXT, lambda s: s.update(agent=AGENT + 4)),
        "slots NULL": (SLOTS_TEXT, lambda s: s.update(slots=None)),
        "slots misaligned": (SLOTS_TEXT, lambda s: s.update(slots=SLOTS + 4)),
        "size 0": ("size must be >= 1 (buffers.py can_sample: nothing is drawn from an empty ring)",
                   lambda s: s.update(size=0)),
    },
    "layout_query": {
        "layout NULL": ("layout is NULL", lambda s: s.update(layout=False)),
    },
}


@pytest.mark.parametrize("what", sorted(OTHER_FAULTS))
def test_the_four_families_other_calls_refuse_alike(L, what):
    assert len(OTHER_CALLS) == 4
    for name, (text, mutate) in OTHER_FAULTS[what].items():
        for fam, prefix in OTHER_CALLS.items():
            assert _other(L, prefix, what, fam, _faulty(mutate)) == text, (prefix + what, name)
    for name, (part, mutate) in PLAN_FAULTS.items():
        for fam, prefix in OTHER_CALLS.items():
            assert part in _other(L, prefix, what, fam, _faulty(mutate)), (prefix + what, name)
