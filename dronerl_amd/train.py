"""The train_jax.py driver over the device env and learner.

`train` is train_jax.py:38-115's scan body run step by step on one GPU (or
one env shard): per step, uniform random actions for every drone, the
epsilon-greedy DQN action for drone 0 (drl_qnet_act_synth, the learner's
device epsilon), the env step writing drone 0's next policy code and landing
the drone-0 transitions in the replay ring (drl_step_code_replay:
buffer.add_many), the learner block (drl_dqn_train: sample + train_step when
the buffer can sample, the target update, the epsilon decay, step + 1; a
conv net: drl_convnet_act and drl_convnet_dqn_train; a dense net wider than
128: drl_widenet_act and drl_widenet_dqn_train; prioritized replay: the
ring wrapped in dqn.PrioritizedReplay and the family's drl_*_dqn_per_train), and
a reset of every env when step % reset_env_every == 0 (:99-113).
`evaluate` is eval_jax (:270-319): greedy drone 0 against random drones,
episodes sharded over ranks with the eval table all-reduced
(distributed.evaluate_sharded).  The trained agent leaves the device in the
reference's formats through DQNLearner.save (train_jax.py:238-244).

The random streams are the build's (counter hashes), not
jax.random's, so a run reproduces this build's runs, not the reference's.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .params import EnvParams


@dataclass
class TrainResult:
    env: object
    net: object
    learner: object
    replay: object
    steps: int
    env_steps_per_s: float


def train(params: EnvParams, num_envs: int, num_steps: int, hidden: Sequence[int] = (128, 64), hp=None,
          reset_env_every: int = 100, memory_size: int = 100_000, seed: int = 0, env_offset: int = 0,
          action_seed: int = 2024, act_seed: int = 7, device=None, rank: int = 0, world: int = 1,
          group=None, network_type: str = "dense", conv_layers=None, conv_dense_layers: Sequence[int] = (),
          per: Optional[dict] = None, double_dqn: bool = False) -> TrainResult:
    """train_jax.py's training loop (see the module docstring).  hp: a
    dqn.DQNHParams (default: train_jax.py's defaults with num_steps, so
    epsilon decays as :133-134 schedules it).  hidden: 1-3 widths, each a
    multiple of 8 in [8, 256] (train_jax.py's default net is (16, 16),
    run_jax_sweep.py's (256, 128, 64)); with a width above 128 the net is a
    dqn.WideQNetwork trained by dqn.WideDQNLearner (one GPU only), otherwise
    today's QNetwork path.  hp.batch (--batch_size): 1..4096 for dense nets
    (dqn.make_learner: the single-launch learner up to 64, the large-batch
    one above; a wide net: the launch chain at every batch) and for conv nets
    (dqn.ConvDQNLearner up to 64, dqn.LargeBatchConvDQNLearner above).

    network_type "conv" (train_jax.py --network_type conv): a ConvQNetwork
    of conv_layers (the reference's tuple of dicts; default train_jax.py's
    one 3x3 layer of 8 channels, padding 1) and conv_dense_layers on the
    policy code, trained by dqn.make_learner's conv learner
    (drl_convnet_dqn_train, or drl_convnet_dqn_large_train above batch 64) in
    the same loop; `hidden` is then unused.  One GPU only (world == 1).

    world > 1 (one process per GPU, an initialised torch.distributed group):
    train_jax.py --use_sharding (:196-212) -- this rank steps envs
    rank * num_envs / world .. (num_envs % world == 0, :401-402), the one
    replay ring is sharded (global_learner.ShardedReplay) and every rank runs
    the same learner; env_offset is then ignored.  The returned rate counts
    every rank's envs.

    per (--prioritized_replay, python -m dronerl_amd.per_train):
    dqn.PrioritizedReplay's keywords (alpha, beta0, beta_steps, eps).  The
    ring is wrapped in a PrioritizedReplay and the learner is
    dqn.make_per_learner's at every batch (PrioritizedDQNLearner, or
    PrioritizedWideDQNLearner, or PrioritizedConvDQNLearner); one GPU only.
    The returned `replay` is the wrapper.

    double_dqn (--double_dqn): the learner's TD target is Double DQN's
    (DQNHParams.double_dqn, set on `hp` here): dense nets of every width, on
    the launch chain at every batch, uniform or prioritized; refused by name
    for conv nets and for world > 1."""
    import dataclasses

    from .dqn import (ConvQNetwork, DQNHParams, PrioritizedReplay, QNetwork, ReplayBuffer, WideQNetwork, is_wide,
                      make_learner, make_per_learner)
    from .distributed import shard_envs
    from .env import BatchedDeliveryDrones
    from .global_learner import ShardedReplay
    if num_steps < 1 or reset_env_every < 1:
        raise ValueError("num_steps and reset_env_every must be >= 1")
    if network_type not in ("dense", "conv"):
        raise ValueError("network_type must be 'dense' or 'conv'")
    if network_type == "conv" and world > 1:
        raise ValueError(CONV_SHARDING_REFUSAL)
    wide = network_type == "dense" and is_wide(hidden)
    if wide and world > 1:
        raise ValueError(WIDE_SHARDING_REFUSAL)
    if per is not None and world > 1:
        raise ValueError(PER_SHARDING_REFUSAL)
    double_dqn = bool(double_dqn or (hp is not None and hp.double_dqn))
    if double_dqn and network_type == "conv":
        raise ValueError(DOUBLE_CONV_REFUSAL)
    if double_dqn and world > 1:
        raise ValueError(DOUBLE_SHARDING_REFUSAL)
    shard = shard_envs(num_envs, rank, world) if world > 1 else None
    env = BatchedDeliveryDrones(params, shard.num_envs if shard else num_envs, device=device,
                                env_offset=shard.env_offset if shard else env_offset)
    env.reset(seed=seed)
    dev, E, N = env.device, env.num_envs, env.n_drones
    r = params.window_radius
    D = (2 * r + 1) ** 2 * 6
    hp = hp or DQNHParams(num_steps=num_steps)
    if double_dqn and not hp.double_dqn:
        hp = dataclasses.replace(hp, double_dqn=True)
    if network_type == "conv":
        from .checkpoint import TRAIN_JAX_CONV_LAYERS
        W = 2 * r + 1
        net = ConvQNetwork((W, W, 6), conv_layers if conv_layers is not None else TRAIN_JAX_CONV_LAYERS,
                           tuple(conv_dense_layers), device=dev, generator=torch.Generator().manual_seed(seed),
                           input="code")
    elif wide:  # (a width above 128: the wide act and the launch-chain learner, dqn.WideDQNLearner)
        net = WideQNetwork(D, tuple(hidden), device=dev, generator=torch.Generator().manual_seed(seed), input="code")
    else:
        net = QNetwork(D, tuple(hidden), device=dev, generator=torch.Generator().manual_seed(seed), input="code")
    # dense: batches up to 64 DQNLearner's one launch, up to 4096 LargeBatchDQNLearner's launch chain (a wide net:
    # the chain at every batch); conv: ConvDQNLearner up to 64, LargeBatchConvDQNLearner's chunked gradients above;
    # prioritized replay: the family's prioritized learner at every batch
    learner = (make_per_learner if per is not None else make_learner)(
        net, hp, generator=torch.Generator().manual_seed(seed + 1))
    if shard:
        rb = ShardedReplay(memory_size, D, dev, num_envs, shard.env_offset, shard.num_envs, rank, world,
                           code_radius=r, group=group)
        ring = rb.ring
    else:
        rb = ring = ReplayBuffer(memory_size, D, dev, code_radius=r)
        if per is not None:  # (the ring with its priority tree: the step's add marks the new rows)
            rb = ring = PrioritizedReplay(rb, batch=hp.batch, **per)
    code = [env.new_code(), env.new_code()]
    env.get_code(out=code[0])
    acts = torch.empty((E, N), dtype=torch.int32, device=dev)
    rew = torch.empty((E, N), dtype=torch.float32, device=dev)
    don = torch.empty((E, N), dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(num_steps):
        b, nb = t & 1, (t + 1) & 1
        # drones 1..N-1 act at random (train_jax.py:42-49): written by the act beside drone 0's action when the
        # step reads them, or drawn by the step itself (drl_step_code_replay_synth; the same counter hash)
        if network_type == "conv" or wide:
            net.act(code[b], learner.epsilon, seed=act_seed, step=t, env_offset=env.env_offset, actions=acts)
        else:
            net.act(code[b], learner.epsilon, seed=act_seed, step=t, env_offset=env.env_offset, actions=acts,
                    synth=(action_seed, t) if shard else None)
        if shard:
            env.step(acts, rewards=rew, dones=don, code=code[nb])
            rb.add_many(code[b], acts, rew, code[nb], don)
            rb.gather(learner)
        else:  # (the step lands its transitions in the ring itself: drl_step_code_replay)
            env.step(acts, rewards=rew, dones=don, code=code[nb], replay=rb, replay_obs=code[b],
                     synth=(action_seed, t))
        learner.train(ring)
        if t % reset_env_every == 0:  # train_jax.py:101-113 (step 0 included)
            env.reset(seed=None)
            env.get_code(out=code[nb])
    e1.record()
    torch.cuda.synchronize(dev)
    env.check_errors()
    net.check_errors()
    learner.check_errors()
    dt = e0.elapsed_time(e1) / 1e3
    if world > 1:
        from .distributed import max_over_ranks
        dt = max_over_ranks(dt, device=dev if torch.distributed.get_backend(group) == "nccl" else None)
    return TrainResult(env, net, learner, ring, num_steps, num_envs * num_steps / dt)


CONV_SHARDING_REFUSAL = ("--use_sharding with --network_type conv is not implemented: the global (sharded) "
                         "learner trains dense nets only")
PER_CONV_REFUSAL = ("--prioritized_replay with --network_type conv is not implemented: prioritized replay trains "
                    "dense nets only")
PER_WIDE_REFUSAL = ("--prioritized_replay with --hidden_layers wider than 128 is not implemented: prioritized replay "
                    "trains dense nets of widths up to 128 only")
PER_SHARDING_REFUSAL = ("--prioritized_replay with --use_sharding is not implemented: the priority tree covers one "
                        "GPU's ring")
DOUBLE_CONV_REFUSAL = ("--double_dqn with --network_type conv is not implemented: Double DQN trains dense nets "
                       "(the conv chains keep the max rule)")
DOUBLE_SHARDING_REFUSAL = ("--double_dqn with --use_sharding is not implemented: the global (sharded) learner keeps "
                           "the max rule")
WIDE_SHARDING_REFUSAL = ("--use_sharding with --hidden_layers wider than 128 is not implemented: the global "
                         "(sharded) learner trains dense nets of widths up to 128 only")


def greedy_policy(qnet):
    """drone 0's greedy action (dqn.act(..., greedy=True), train_jax.py:286)
    from a QNetwork on f32 observation rows."""

    def policy(obs: torch.Tensor) -> torch.Tensor:
        return qnet.act(obs, 0.0)[:, 0]

    return policy


def evaluate(params: EnvParams, qnet, num_evals: int = 5, num_eval_steps: int = 10_000, eval_seed: int = 0,
             rank: int = 0, world: int = 1, device=None):
    """eval_jax (train_jax.py:270-319): `num_evals` episodes of
    `num_eval_steps` steps, episode i seeded eval_seed + i, drone 0 greedy,
    every other drone uniform random; episodes sharded over ranks and the
    table all-reduced.  Returns ((mean, std) agent, (mean, std) random, table)."""
    from .distributed import evaluate_sharded, gpu_episode_runner
    run = gpu_episode_runner(params, num_eval_steps, eval_seed, policy=greedy_policy(qnet), action_seed=eval_seed,
                             device=device)
    return evaluate_sharded(run, num_evals, rank, world, device=device)


def parse_args(argv=None):
    """train_jax.py's command line (:335-390) for the options this driver
    implements: the env, training and eval options and
    --save_final_checkpoint; the dense net's widths are multiples of 8 in
    [8, 256] (1-3 layers), so train_jax.py's default `--hidden_layers 16 16`
    and run_jax_sweep.py's `256 128 64` run as they are (a width above 128:
    the wide path, dqn.WideQNetwork; not with --use_sharding).
    --hidden_layers here defaults to the benchmark net (128, 64): a choice
    (what this command has always trained), no longer a limit of the device
    act.  --use_sharding runs under torchrun (one process per GPU)."""
    import argparse
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--n_drones", type=int, default=4)
    ap.add_argument("--grid_size", type=int, default=9)
    ap.add_argument("--window_radius", type=int, default=3)
    ap.add_argument("--packets_factor", type=int, default=3)
    ap.add_argument("--dropzones_factor", type=int, default=2)
    ap.add_argument("--stations_factor", type=int, default=2)
    ap.add_argument("--skyscrapers_factor", type=int, default=3)
    ap.add_argument("--num_envs", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_steps", type=int, default=1000)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--learning_rate", type=float, default=1e-3)
    ap.add_argument("--memory_size", type=int, default=100_000)
    ap.add_argument("--epsilon_start", type=float, default=1.0)
    ap.add_argument("--epsilon_decay", type=float, default=None)
    ap.add_argument("--epsilon_decay_half_life_fraction", type=float, default=0.2)
    ap.add_argument("--epsilon_end", type=float, default=0.01)
    ap.add_argument("--epsilon_decay_every", type=int, default=5)
    ap.add_argument("--target_update_interval", type=int, default=10)
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--reset_env_every", type=int, default=100)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--save_final_checkpoint", action="store_true", default=False)
    ap.add_argument("--use_sharding", action="store_true", default=False)
    ap.add_argument("--network_type", choices=["dense", "conv"], default="dense")
    ap.add_argument("--hidden_layers", nargs="+", type=int, default=(128, 64), help="dense network hidden layer sizes")
    ap.add_argument("--conv_layers", type=_parse_conv_layers,
                    default='[{"kernel_size": 3, "out_channels": 8, "padding": 1, "stride": 1}]',
                    help="conv network config (stringified JSON)")
    ap.add_argument("--conv_dense_layers", nargs="+", type=int, default=(),
                    help="conv network: hidden dense layer sizes after the convolutions")
    ap.add_argument("--pickup_reward", type=float, default=0.0)
    ap.add_argument("--delivery_reward", type=float, default=1.0)
    ap.add_argument("--crash_reward", type=float, default=-1.0)
    ap.add_argument("--charge_reward", type=float, default=-0.1)
    ap.add_argument("--eval_n_drones", type=int, default=None)
    ap.add_argument("--eval_grid_size", type=int, default=None)
    ap.add_argument("--eval_seed", type=int, default=0)
    ap.add_argument("--num_eval_steps", type=int, default=10_000)
    ap.add_argument("--num_evals", type=int, default=5)
    ap.add_argument("--output_dir", default="output")
    ap.add_argument("--prioritized_replay", action="store_true", default=False,
                    help="draw the replay rows by priority (proportional prioritized replay on the device)")
    ap.add_argument("--per_alpha", type=float, default=0.6, help="priority = (|td error| + per_eps) ** per_alpha")
    ap.add_argument("--per_beta", type=float, default=0.4, help="the importance exponent at step 0")
    ap.add_argument("--per_beta_steps", type=int, default=None,
                    help="learner steps over which beta anneals to 1 (default: num_steps; 0: per_beta throughout)")
    ap.add_argument("--per_eps", type=float, default=1e-6)
    ap.add_argument("--double_dqn", action="store_true", default=False,
                    help="Double DQN targets: the target net's value at the online net's argmax on next_obs")
    args = ap.parse_args(argv)
    # train_jax.py:393-402's validations
    if args.num_envs <= 0:
        raise ValueError("Number of envs need to be at least 1")
    if args.num_steps <= 0:
        raise ValueError("Number of steps need to be at least 1")
    if args.use_sharding and args.num_envs <= 1:
        raise ValueError("When using --use_sharding you need to provide num_envs > 1")
    if args.use_sharding and args.network_type == "conv":
        raise ValueError(CONV_SHARDING_REFUSAL)
    if args.use_sharding and args.network_type == "dense" and max(args.hidden_layers) > 128:
        raise ValueError(WIDE_SHARDING_REFUSAL)
    if args.double_dqn and args.network_type == "conv":
        raise ValueError(DOUBLE_CONV_REFUSAL)
    if args.double_dqn and args.use_sharding:
        raise ValueError(DOUBLE_SHARDING_REFUSAL)
    if args.per_beta_steps is None:
        args.per_beta_steps = args.num_steps  # (the usual anneal to 1 over the run)
    if args.prioritized_replay:
        if args.network_type == "conv":
            raise ValueError(PER_CONV_REFUSAL)
        if max(args.hidden_layers) > 128:
            raise ValueError(PER_WIDE_REFUSAL)
        if args.use_sharding:
            raise ValueError(PER_SHARDING_REFUSAL)
        if args.per_alpha < 0 or not 0 <= args.per_beta <= 1 or args.per_beta_steps < 0 or args.per_eps < 0:
            raise ValueError("--per_alpha and --per_eps must be >= 0, --per_beta in [0, 1], --per_beta_steps >= 0")
    return args


def per_options_of(args) -> Optional[dict]:
    """PrioritizedReplay's keywords from the command line (None: uniform replay)."""
    if not args.prioritized_replay:
        return None
    return dict(alpha=args.per_alpha, beta0=args.per_beta, beta_steps=args.per_beta_steps, eps=args.per_eps)


def refuse_prioritized(args, driver: str):
    """The drivers that train several learners draw uniformly: --prioritized_replay is refused by name."""
    if getattr(args, "prioritized_replay", False):
        raise ValueError(f"--prioritized_replay is not implemented for {driver}: it trains one dense agent "
                         "(python -m dronerl_amd.train)")


def refuse_double_dqn(args, driver: str, points=()):
    """The drivers whose learners keep the max rule refuse --double_dqn by
    name, on the command line and as a --grid key (`points`)."""
    if getattr(args, "double_dqn", False) or any("double_dqn" in pt for pt in points):
        raise ValueError(f"--double_dqn is not implemented for {driver}: Double DQN trains dense single agents "
                         "(python -m dronerl_amd.train, per_train) and dense populations (python -m dronerl_amd.sweep)")


def _parse_conv_layers(value: str):
    """train_jax.py:323-334: stringified JSON (or a Python literal) -> a tuple of dicts."""
    import argparse
    import ast
    import json
    try:
        layers = json.loads(value)
    except json.JSONDecodeError:
        try:
            layers = ast.literal_eval(value)
        except (SyntaxError, ValueError):
            raise argparse.ArgumentTypeError(f"Invalid format for conv_layers: {value}.")
    return (layers,) if isinstance(layers, dict) else tuple(layers)


def env_params_of(args, eval_env: bool = False) -> EnvParams:
    n = args.eval_n_drones if eval_env and args.eval_n_drones is not None else args.n_drones
    g = args.eval_grid_size if eval_env and args.eval_grid_size is not None else args.grid_size
    return EnvParams(n_drones=n, grid_size=g, window_radius=args.window_radius, pickup_reward=args.pickup_reward,
                     delivery_reward=args.delivery_reward, crash_reward=args.crash_reward,
                     charge_reward=args.charge_reward, packets_factor=args.packets_factor,
                     dropzones_factor=args.dropzones_factor, stations_factor=args.stations_factor,
                     skyscrapers_factor=args.skyscrapers_factor)


def hparams_of(args):
    from .dqn import DQNHParams
    if args.epsilon_decay is None:  # train_jax.py:133-134
        decay = (1 - 0.5 * (1 - args.epsilon_end / args.epsilon_start)) ** (
            1 / (args.epsilon_decay_half_life_fraction * args.num_steps))
    else:
        decay = args.epsilon_decay
    return DQNHParams(batch=args.batch_size, gamma=args.gamma, learning_rate=args.learning_rate, tau=args.tau,
                      target_update_interval=args.target_update_interval, epsilon_start=args.epsilon_start,
                      epsilon_decay=decay, epsilon_end=args.epsilon_end,
                      epsilon_decay_every=args.epsilon_decay_every, num_steps=args.num_steps,
                      sample_seed=args.seed, double_dqn=bool(getattr(args, "double_dqn", False)))


def main(argv=None) -> dict:
    """`python -m dronerl_amd.train [train_jax.py options]`: train, save
    (train_jax.py:238-244: agent_<n>_steps_jax / _torch.safetensors under
    output/jax_run_<time>), evaluate (:247-256).  Returns the metrics."""
    return run(parse_args(argv))


def run(args) -> dict:
    """`main` behind the command line: `args` is parse_args' result
    (dronerl_amd.per_train passes its own, with prioritized replay on)."""
    import json
    import os
    from datetime import datetime

    from .distributed import init_from_env
    rank, world, local = init_from_env() if args.use_sharding else (0, 1, 0)
    if args.use_sharding and args.num_envs % world:
        raise ValueError(f"The number of envs (={args.num_envs}) needs to be divisible by the number of devices "
                         f"(={world})")
    dev = torch.device("cuda", local if world > 1 else torch.cuda.current_device())
    res = train(env_params_of(args), args.num_envs, args.num_steps, hidden=tuple(args.hidden_layers),
                hp=hparams_of(args), reset_env_every=args.reset_env_every, memory_size=args.memory_size,
                seed=args.seed, device=dev, rank=rank, world=world, network_type=args.network_type,
                conv_layers=args.conv_layers, conv_dense_layers=tuple(args.conv_dense_layers),
                per=per_options_of(args))
    metrics = {"obs_per_sec": res.env_steps_per_s, "time_taken": args.num_envs * args.num_steps / res.env_steps_per_s,
               "num_gpus": world}
    run_dir = os.path.join(args.output_dir, f"jax_run_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    if args.save_final_checkpoint and rank == 0:
        os.makedirs(run_dir, exist_ok=True)
        for fmt in ("jax", "torch"):
            path = os.path.join(run_dir, f"agent_{args.num_steps}_steps_{fmt}.safetensors")
            if args.network_type == "conv":  # (the metadata train_jax.py writes: its options as given)
                res.learner.save(path, format=fmt, conv_layers=args.conv_layers,
                                 hidden_layers=tuple(args.hidden_layers))
            else:
                res.learner.save(path, format=fmt)
            metrics[f"checkpoint_{fmt}"] = path
    # the final eval with the trained net (the online parameters, as eval_jax uses ag_state)
    from .dqn import ConvQNetwork, QNetwork, WideQNetwork
    if args.network_type == "conv":
        qnet = ConvQNetwork(res.net.obs_shape, res.net.conv_layers, res.net.dense_layers, device=dev)
        qnet.load(res.net.conv_weights, res.net.conv_biases, res.net.weights, res.net.biases)
    elif isinstance(res.net, WideQNetwork):
        qnet = WideQNetwork(res.net.in_features, res.net.hidden, device=dev)
        qnet.load(*zip(*res.learner.params("online")))
    else:
        qnet = QNetwork(res.net.in_features, res.net.hidden, device=dev, precision="f32")
        qnet.load(*zip(*res.learner.params("online")))
    (am, asd), (rm, rsd), _ = evaluate(env_params_of(args, eval_env=True), qnet, args.num_evals, args.num_eval_steps,
                                      args.eval_seed, rank=rank, world=world, device=dev)
    metrics.update(eval_reward_mean=am, eval_reward_std=asd, random_reward_mean=rm, random_reward_std=rsd)
    if rank == 0:
        print(json.dumps(metrics), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()
    return metrics


if __name__ == "__main__":
    main()
