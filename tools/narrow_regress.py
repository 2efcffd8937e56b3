#!/usr/bin/env python3
"""(128, 64) at C3: this tree's library against another checkout's (--other ROOT, e.g. `git worktree add` of
the parent commit, built there with `python -m dronerl_amd.build`), both packages loaded in one process and
alternating repeat by repeat: code act, f32 obs act, learner step (device events around 200 launches per
repeat); plus byte comparisons of packed sizes, learner layouts, images, Q and the learner's state
(profiles/narrow_nets/regress_128_64.json).  Writes the JSON to --out."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def load_pkg(name, root):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "dronerl_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(root, "dronerl_amd")])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True, help="root of the other checkout (built)")
ap.add_argument("--out", default="regress_128_64.json")
ap.add_argument("--other-first", action="store_true", help="time the other checkout first in every pair (an offset that follows the position, not the library, is the measurement's)")
args = ap.parse_args()
new = load_pkg("dronerl_amd", REPO)
old = load_pkg("dronerl_parent", os.path.abspath(args.other))
import dronerl_amd.dqn as ndqn  # noqa: E402
import dronerl_parent.dqn as odqn  # noqa: E402
import dronerl_parent._native as onat  # noqa: E402
import dronerl_amd._native as nnat  # noqa: E402
assert onat.LIB_PATH != nnat.LIB_PATH, (onat.LIB_PATH, nnat.LIB_PATH)

E, ITERS, REPS = 65536, 200, 7
out = {"order": "other first" if args.other_first else "this tree first"}

# ---- layouts of widths that are multiples of 32: the same bytes
same_sizes = True
for hidden in ((128, 64), (32, 32), (64,), (128, 128, 128), (96, 32), (64, 64, 32), (32, 128, 128)):
    for prec in (0, 1):
        for inp in (0, 1):
            if inp == 1 and prec == 0:
                continue
            vals = []
            for mod in (ndqn, odqn):
                L = mod._bind(mod.lib())
                h = list(hidden) + [0] * (3 - len(hidden))
                d = mod.DrlQnetDesc(294, len(hidden), (ctypes.c_int32 * 3)(*h), 5, prec, inp)
                nb = ctypes.c_int64()
                rc = L.drl_qnet_packed_bytes(ctypes.byref(d), ctypes.byref(nb))
                lay = mod.DrlDqnLayout()
                rc2 = L.drl_dqn_layout_query(ctypes.byref(d), 8, ctypes.byref(lay))
                vals.append((rc, nb.value, rc2, bytes(lay)))
            same_sizes &= vals[0] == vals[1]
out["sizes_and_learner_layouts_identical"] = same_sizes

envs = {}
for tag, pkg in (("new", new), ("parent", old)):
    env = pkg.BatchedDeliveryDrones(pkg.EnvParams(n_drones=8, grid_size=16), E)
    env.reset(seed=0)
    code = env.new_code()
    for t in range(6):
        _, _, obs = env.step(env.synth_actions(seed=1, step=t), obs_k=1, code=code)
    envs[tag] = (env, code, obs.reshape(E, -1).contiguous())
assert torch.equal(envs["new"][1], envs["parent"][1])
acts = torch.zeros((E, 8), dtype=torch.int32, device="cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(ITERS):
        fn(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def ab(name, fns):
    order = list(fns)[::-1] if args.other_first else list(fns)
    for tag in order:
        for _ in range(3):
            timed(fns[tag])
    ts = {tag: [] for tag in fns}
    for r in range(REPS):
        for tag in order:
            ts[tag].append(timed(fns[tag]))
    out[name] = {tag: {"us": [round(v, 3) for v in ts[tag]], "median": round(statistics.median(ts[tag]), 3),
                       "max_minus_min": round(max(ts[tag]) - min(ts[tag]), 3)} for tag in fns}


# ---- acts
for name, inp in (("act_code_128_64_c3_65536", "code"), ("act_f32_obs_128_64_c3_65536", "obs")):
    nets, qs = {}, {}
    for tag, mod in (("new", ndqn), ("parent", odqn)):
        net = mod.QNetwork(294, (128, 64), generator=torch.Generator().manual_seed(0), precision="f32", input=inp)
        net.packed.fill_(0x7F7F7F7F)
        net.pack()
        nets[tag] = net
        q = torch.empty((E, 5), device="cuda")
        src = envs[tag][1] if inp == "code" else envs[tag][2]
        a = net.act(src, 0.0, q_out=q).clone()
        qs[tag] = (q, a)
    out[name + "_image_identical"] = bool(torch.equal(nets["new"].packed, nets["parent"].packed))
    out[name + "_q_identical"] = bool(torch.equal(qs["new"][0], qs["parent"][0]) and
                                      torch.equal(qs["new"][1], qs["parent"][1]))
    ab(name, {tag: (lambda t, n=nets[tag], s=(envs[tag][1] if inp == "code" else envs[tag][2]):
                    n.act(s, 0.1, step=t, actions=acts)) for tag in nets})

# ---- learner: a filled code ring, train_jax defaults
lrs = {}
for tag, mod in (("new", ndqn), ("parent", odqn)):
    env, code, _ = envs[tag]
    net = mod.QNetwork(294, (128, 64), generator=torch.Generator().manual_seed(0), input="code")
    lr = mod.DQNLearner(net, mod.DQNHParams(num_steps=1000), generator=torch.Generator().manual_seed(1))
    rb = mod.ReplayBuffer(100_000, 294, torch.device("cuda"), code_radius=3)
    nxt = env.new_code()
    a = env.synth_actions(seed=3, step=0)
    r, d = env.step(a, code=nxt)
    rb.add_many(code, a, r, nxt, d)
    lrs[tag] = (lr, rb, net)
ab("learner_128_64_batch8", {tag: (lambda t, l=lrs[tag][0], b=lrs[tag][1]: l.train(b)) for tag in lrs})
same = True
for k in ("online", "target", "m", "v"):
    for (w0, b0), (w1, b1) in zip(lrs["new"][0].params(k), lrs["parent"][0].params(k)):
        same &= bool(torch.equal(w0, w1) and torch.equal(b0, b1))
same &= bool(torch.equal(lrs["new"][2].packed, lrs["parent"][2].packed))
same &= lrs["new"][0].counters() == lrs["parent"][0].counters()
out["learner_state_and_image_identical_after_steps"] = same
out["learner_steps"] = lrs["new"][0].counters()["step"]
for tag in lrs:
    lrs[tag][0].check_errors()

with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
