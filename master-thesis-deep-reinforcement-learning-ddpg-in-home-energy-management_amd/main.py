"""The reference's entry point, RL-SHEMS/DDPG_reinforce_charger_v1.jl, on the GPU-resident path.

Process contract kept from the reference (MAIN = DDPG_reinforce_charger_v1.jl, INPUT = input.jl / the job's input template):
    JOB_ID    MAIN:10   digits 3-4 from the right = charger id (INPUT:38, LU1:45); last two digits = hyper-parameter code
              (ternary, `set_hyperparameters`, input_templates/input09_08_on_01-09_eval.jl:62-106)
    TASK_ID   INPUT:35-36  seed_run; rng_run = parse(Int, "123" * TASK_ID) (INPUT:135-136)
    GPU_ID    MAIN:12-14   device index
    data      data/<Charger_ID>_<season>_<split>_<price>.csv (INPUT:162-164), relative to the working directory
    outputs   out/bson/[temp/]DDPG_Shems_Charger_v1_<EP>_<NUM_EP>_<L1>_<L2>_<case>_<rng>_{actor,scores}_<idx>   (MPS:263-268)
              out/tracker/<Job_ID>_<run>_results_charger_v1_<EP>_<NUM_EP>_<L1>_<L2>_<case>_<rng>_<idx|best>.csv (MPS:167-190)
              out/Tracker_Charger.csv                                                                          (MPS:193-212)
Order of MAIN:28-110: populate_memory -> min_max_buffer -> run_episodes (best-score snapshots under out/bson/temp) -> saveBSON ->
(the last seed of the job) inference + write_to_results_file + write_to_tracker_file for every seed's last and best actor.

Differences that follow from the platform, all explicit:
  * the job's Julia input file (out/input/$JOB_ID--input.jl) cannot be executed; its decoding rules are restated here for the two
    templates the thesis used last (TUNED = input09_08_on_01-09_eval.jl and input.jl), selected with SHEMS_INPUT_TEMPLATE;
  * the kernels are built for the tuned architecture (L1, L2) = (250, 500) and 128 minibatch columns; the grids' other points run
    too: smaller networks zero-padded, (300, 600) layer by layer (csrc/shems_wide.hip), BATCH_SIZE 150 / 200 as sub-batches;
  * snapshots are BSON files under the reference's names, laid out as BSON.jl lowers a Chain (bson_chain.py; parity unpinned:
    the reference ships no real .bson to compare with);
  * SHEMS_NUM_ENVS (default 1 = the reference's protocol) trains that many households at once;
  * SHEMS_ALGO=td3[:d[:sigma_trg[:clip_trg]]] trains a td3.TD3Agent (twin critics, target smoothing, the actor every d-th update;
    defaults 2, 0.2, 0.5) and appends _td3-d<d>-s<sigma>-c<clip> to <case>; unset or `ddpg`: today's bytes and file names;
  * SHEMS_REPLAY=per[:alpha[:beta0]] trains from a replay.PrioritizedRing (proportional prioritized replay, beta annealed from beta0
    to 1 over the run; defaults 0.6, 0.4) and appends _per-a<alpha>-b<beta0> to <case>; unset or `uniform`: today's bytes and names;
  * SHEMS_NSTEP=<n> (1 .. 16) trains on multi-step returns (Agent(n_step=n): n-step transitions, y = G + gamma^n q') and appends _n<n>
    to <case>, behind the suffixes above; it combines with SHEMS_ALGO=td3 and SHEMS_REPLAY=per; unset or 1: today's bytes and names;
  * SHEMS_BC=<alpha>[:<weight>] trains with the behaviour-regularised actor loss of TD3+BC (ddpg.BC; weight default 1) and appends
    _bc-a<alpha>-w<weight> to <case>, behind the suffixes above; it combines with SHEMS_ALGO=td3 and SHEMS_NSTEP, not with
    SHEMS_REPLAY=per; unset: today's bytes and names; SHEMS_FORESIGHT_OFFLINE=<updates> (needs SHEMS_FORESIGHT=1 and SHEMS_BC) first
    trains offline on the foresight pass of the training series (imitation.offline) and writes ..._results_<case>_offline.csv;
  * SHEMS_FORESIGHT=1 adds, after the tracking block, the perfect-foresight pass over the tracked data set (foresight.py):
    out/tracker/<Job_ID>_<run>_results_<case>_foresight.csv and a tracker row with seed = "foresight"; with it,
    SHEMS_FORESIGHT_HORIZON (hours of forecast: one integer or a comma list) and SHEMS_FORESIGHT_CONTROL (hours between plans,
    default 1) add one receding-horizon pass per horizon: ..._foresight_h24.csv / ..._foresight_h24_c12.csv, seed = that suffix;
    SHEMS_FORESIGHT_FORECAST=persistence[:LAG[:ev]] (needs a horizon; LAG default 24 hours) adds, after each of those, the same
    controller planning on the persistence forecast of load and PV -- with `ev` of h_countdown and soc_ev too --:
    ..._foresight_h24_p24.csv / ..._foresight_h24_p24ev.csv; SHEMS_FORESIGHT_FORECAST=analog:24,48,72[:ev] instead adds the controller
    that hedges over the analog ensemble of those lags with equal weights (foresight.solve_ensemble): ..._foresight_h24_a24-48-72.csv;
    SHEMS_FORESIGHT_IMITATE=<rounds>x<steps> (needs SHEMS_FORESIGHT=1) trains a fresh actor by imitation of the foresight pass
    (imitation.dagger) and writes its per-round figures to ..._results_<case>_imitation.csv;
    SHEMS_FORESIGHT_WARMSTART=<critic_steps>[:td|:mc] (needs SHEMS_FORESIGHT_IMITATE) then fits the same agent's critic on the
    transitions of one pass of the cloned actor (imitation.warm_start) and writes ..._results_<case>_warmstart.csv;
    SHEMS_FORESIGHT_REGRET=1 (needs SHEMS_FORESIGHT=1) adds one <results file>_regret.csv next to every results file of the tracking
    block -- the hourly regret of that pass against ONE perfect-foresight solve (harness.regret_of; the forecast passes are audited
    against the truth like the rest);
  * random streams are Philox counters keyed by the same seeds (Julia's MersenneTwister streams do not exist outside Julia).
"""
from __future__ import annotations

import dataclasses
import math
import os
import sys
import time

import numpy as np

SEED_INI = 123                                   # INPUT:134
EP_LENGTH = {"train": 72, ("all", "eval"): 1439, ("all", "test"): 2999, ("summer", "eval"): 359, ("summer", "test"): 767,
             ("winter", "eval"): 359, ("winter", "test"): 719, ("both", "eval"): 719, ("both", "test"): 1487}   # INPUT:154-160


def julia_float(x, f32=True):
    """How Julia's string interpolation prints a Float32 / Float64 value (`$(x)`): the shortest digits that round-trip, in fixed
    notation when the decimal exponent of that shortest form is in [-4, 21) (always with a decimal point: 0.0001, 24000.0), otherwise
    as d.ddde-N (1.0e-5).  Needed for the `case` string in every file name."""
    v = np.float32(x) if f32 else np.float64(x)
    if v == 0:
        return "0.0"
    mant, exp = np.format_float_scientific(v, unique=True, trim="0", exp_digits=1).split("e")
    if -4 <= int(exp) < 21:
        r = np.format_float_positional(v, unique=True, trim="0")
        return r if "." in r else r + ".0"
    if "." not in mant:
        mant += ".0"
    return f"{mant}e{int(exp)}"


@dataclasses.dataclass
class RunConfig:
    job_id: str
    task_id: str
    gpu_id: int
    template: str = "tuned"
    train: int = 1
    track: float = 1                             # 0 off, 1 DRL, < 0 rule-based (INPUT:47)
    run: str = "eval"
    season: str = "all"
    price: str = "fix"
    num_seeds: int = 40
    test_every: int = 100
    test_runs: int = 100
    # hyper-parameters (filled by set_hyperparameters)
    L1: int = 250
    L2: int = 500
    gamma: float = 0.99
    tau: float = 1e-3
    eta_act: float = 1e-4
    eta_crit: float = 1e-3
    sigma: float = 0.1
    theta: float = 0.15
    noise_act: float = 0.1
    noise_trg: float = 0.2
    DISCOMFORT_WEIGHT_EV: float = 0.01
    penalty: float = 0.1
    TRAIN_EP_LENGTH: int = 72
    NUM_EP: int = 1001
    BATCH_SIZE: int = 120
    MEM_SIZE: int = 24000
    noise_type: str = "gn"
    algo_suffix: str = ""                        # SHEMS_ALGO=td3...: "_td3-d<d>-s<sigma>-c<clip>" (td3.case_suffix); DDPG: nothing

    @property
    def charger_id(self):
        return (int(self.job_id) // 100) % 100          # INPUT:38, LU1:45

    @property
    def Charger_ID(self):
        return "Charger%02d" % self.charger_id

    @property
    def seed_run(self):
        return int(self.task_id)

    @property
    def rng_run(self):
        return int(str(SEED_INI) + str(self.seed_run))   # INPUT:136

    @property
    def case(self):
        return self._case_ddpg + self.algo_suffix

    @property
    def _case_ddpg(self):
        if self.track < 0:                               # INPUT:143-144
            return f"{self.Charger_ID}_rule_based_{julia_float(self.track, f32=False) if self.track != int(self.track) else int(self.track)}"
        f = julia_float
        if self.template == "tuned":                     # TUNED:155
            return (f"{self.Charger_ID}_dw{f(self.DISCOMFORT_WEIGHT_EV, False)}_p{f(self.penalty, False)}_B{self.BATCH_SIZE}_M{self.MEM_SIZE}_"
                    f"{self.noise_type}-o{f(self.sigma)}_th{f(self.theta)}_Y{f(self.gamma)}_tau{f(self.tau)}_lract{f(self.eta_act)}_"
                    f"lrcrit{f(self.eta_crit)}_nact{f(self.noise_act)}_ntrg{f(self.noise_trg)}")
        dw = self.DISCOMFORT_WEIGHT_EV                   # INPUT:146 (Int 2 / Float64 0.5 in that template)
        return (f"{self.Charger_ID}_disw{dw if isinstance(dw, int) else f(dw, False)}_pen{f(self.penalty, False)}_BATCH{self.BATCH_SIZE}_"
                f"MEM{self.MEM_SIZE}_{self.noise_type}-noise_om{f(self.sigma)}_th{f(self.theta)}_Y{f(self.gamma)}_tau{f(self.tau)}_"
                f"nact{f(self.eta_act)}_ncrit{f(self.eta_crit)}_smart-trainEP")


def set_hyperparameters(cfg: RunConfig):
    """`set_hyperparameters(Job_ID)`: the last two digits of JOB_ID in base 3 pick one of three alternatives per hyper-parameter."""
    code = int(cfg.job_id[-2:])
    if cfg.template == "tuned":                          # TUNED:62-106: 4 ternary digits -> BATCH, noise_act, (L1, L2), (eta_act, eta_crit)
        alt = {1: (120, 100, 150), 2: (0.1, 0.2, 0.3), 3: ((300, 600), (200, 400), (250, 500)), 4: ((1e-5, 1e-4), (5e-4, 5e-3), (1e-4, 1e-3))}
        cfg.L1, cfg.L2 = alt[3][0]
        cfg.eta_act, cfg.eta_crit = alt[4][0]
        cfg.BATCH_SIZE, cfg.noise_act = alt[1][0], alt[2][0]
        cfg.gamma, cfg.tau, cfg.sigma, cfg.theta = 0.99, 1e-3, 0.1, 0.15
        cfg.DISCOMFORT_WEIGHT_EV, cfg.penalty, cfg.NUM_EP, cfg.MEM_SIZE, cfg.noise_type, cfg.noise_trg = 0.01, 0.1, 1001, 24000, "gn", 0.2
        digits = np.base_repr(code, 3).zfill(4)
        if len(digits) > 4:
            raise ValueError(f"JOB_ID suffix {code} has more than four ternary digits")
        for i, ch in enumerate(digits, start=1):
            d = int(ch)
            if i == 4:
                cfg.eta_act, cfg.eta_crit = alt[4][d]
            elif i == 3:
                cfg.L1, cfg.L2 = alt[3][d]
            elif i == 2:
                cfg.noise_act = alt[2][d]
            else:
                cfg.BATCH_SIZE = alt[1][d]
        cfg.num_seeds = 40                               # TUNED:55
    elif cfg.template == "input":                        # INPUT:58-100: 3 ternary digits -> MEM_SIZE, BATCH_SIZE, (L1, L2, gamma, sigma, theta)
        alt = {1: (30000, 20000, 24000), 2: (200, 50, 120),
               3: ((150, 300, 0.99, 0.1, 0.15), (300, 600, 0.999, 0.1, 0.15), (300, 600, 0.99, 0.2, 0.2))}
        cfg.L1, cfg.L2, cfg.gamma, cfg.sigma, cfg.theta = alt[3][0]
        cfg.tau, cfg.eta_act, cfg.eta_crit = 1e-3, 1e-4, 1e-3
        cfg.DISCOMFORT_WEIGHT_EV, cfg.penalty, cfg.NUM_EP, cfg.noise_type = 2, 0.5, 101, "ou"
        cfg.BATCH_SIZE, cfg.MEM_SIZE = alt[2][0], alt[1][0]
        digits = np.base_repr(code, 3).zfill(3)
        for i, ch in enumerate(digits, start=1):
            d = int(ch)
            if i == 3:
                cfg.L1, cfg.L2, cfg.gamma, cfg.sigma, cfg.theta = alt[3][d]
            elif i == 2:
                cfg.BATCH_SIZE = alt[2][d]
            else:
                cfg.MEM_SIZE = alt[1][d]
        cfg.noise_act, cfg.noise_trg = 0.1, 0.2          # INPUT:230-231
        cfg.num_seeds = 2                                # INPUT:52
    else:
        raise ValueError(f"unknown input template {cfg.template!r} (tuned | input)")
    return cfg


def config_from_env(environ=os.environ):
    """MAIN:10-14 + INPUT:34-52.  SHEMS_* variables are this build's additions (test-sized runs, batch width, template)."""
    for k in ("JOB_ID", "TASK_ID", "GPU_ID"):
        if k not in environ:
            raise KeyError(f"{k} is not set (the reference reads ENV[\"{k}\"], DDPG_reinforce_charger_v1.jl:10-14 / input.jl:34-36)")
    cfg = RunConfig(job_id=str(environ["JOB_ID"]), task_id=str(environ["TASK_ID"]), gpu_id=int(environ["GPU_ID"]),
                    template=environ.get("SHEMS_INPUT_TEMPLATE", "tuned"))
    set_hyperparameters(cfg)
    for name, cast in (("NUM_EP", int), ("num_seeds", int), ("test_every", int), ("test_runs", int), ("track", float), ("train", int),
                       ("run", str)):
        v = environ.get("SHEMS_" + name.upper())
        if v is not None:
            setattr(cfg, name, cast(v))
    return cfg


def parse_replay(value):
    """SHEMS_REPLAY -> ("uniform", None) when unset or "uniform": today's bytes and file names.  per[:alpha[:beta0]] -> ("per",
    dict(alpha, beta0)): a replay.PrioritizedRing with beta annealed linearly from beta0 to 1 over the run (defaults 0.6, 0.4).
    Anything else is refused by name."""
    if value is None or value == "uniform":
        return "uniform", None
    parts = str(value).split(":")
    if parts[0] != "per" or len(parts) > 3:
        raise ValueError(f"SHEMS_REPLAY = {value!r} is not uniform or per[:alpha[:beta0]]")
    out = dict(alpha=0.6, beta0=0.4)
    try:
        for key, raw in zip(("alpha", "beta0"), parts[1:]):
            out[key] = float(raw)
    except ValueError:
        raise ValueError(f"SHEMS_REPLAY = {value!r}: alpha and beta0 are numbers") from None
    if not (math.isfinite(out["alpha"]) and out["alpha"] >= 0.0):
        raise ValueError(f"SHEMS_REPLAY = {value!r}: alpha must be finite and >= 0")
    if not (math.isfinite(out["beta0"]) and 0.0 <= out["beta0"] <= 1.0):
        raise ValueError(f"SHEMS_REPLAY = {value!r}: beta0 must be in [0, 1]")
    return "per", out


def replay_case_suffix(alpha, beta0):
    """What the entry script appends to its `case` string for a prioritized run, behind the algorithm's own suffix."""
    return f"_per-a{float(alpha):g}-b{float(beta0):g}"


def parse_nstep(value):
    """SHEMS_NSTEP -> the steps of a multi-step return: 1 when unset or "1" (today's bytes and file names), else an integer in 2 .. 16
    (replay.NSTEP_MAX).  Anything else is refused by name."""
    if value is None:
        return 1
    raw = str(value).strip()
    if not (raw.isascii() and raw.isdigit()) or not 1 <= int(raw) <= 16:
        raise ValueError(f"SHEMS_NSTEP = {value!r} is not an integer in 1 .. 16")
    return int(raw)


def nstep_case_suffix(n_step):
    """What the entry script appends to its `case` string for an n-step run, behind the algorithm's and the replay's suffixes."""
    return "" if int(n_step) == 1 else f"_n{int(n_step)}"


def nstep_from_env(environ=os.environ):
    return parse_nstep(environ.get("SHEMS_NSTEP"))


def replay_from_env(environ=os.environ):
    return parse_replay(environ.get("SHEMS_REPLAY"))


def algo_from_env(environ=os.environ):
    """SHEMS_ALGO = ddpg (or unset) -> ("ddpg", None): today's bytes and file names.  td3[:d[:sigma_trg[:clip_trg]]] -> ("td3",
    dict(policy_delay, sigma_trg, clip_trg)) (defaults 2, the input's noise_trg = 0.2, 0.5): a td3.TD3Agent is trained and the `case`
    string gains _td3-d<d>-s<sigma>-c<clip>.  Any other value or a malformed field is refused by name."""
    from .td3 import parse_algo
    return parse_algo(environ.get("SHEMS_ALGO"))


def foresight_horizons(environ=os.environ):
    """SHEMS_FORESIGHT_HORIZON (one integer or a comma list, each >= 1) and SHEMS_FORESIGHT_CONTROL (one integer, default 1, at most
    the smallest horizon) -> ([horizons], control); ([], 1) when no horizon is named.  A malformed value is refused by name."""
    raw, raw_c = environ.get("SHEMS_FORESIGHT_HORIZON"), environ.get("SHEMS_FORESIGHT_CONTROL")
    try:
        control = 1 if raw_c is None else int(raw_c)
    except ValueError:
        raise ValueError(f"SHEMS_FORESIGHT_CONTROL = {raw_c!r} is not an integer") from None
    if control < 1:
        raise ValueError(f"SHEMS_FORESIGHT_CONTROL = {raw_c!r}: a fresh plan every 1 or more hours")
    if raw is None:
        if raw_c is not None:
            raise ValueError("SHEMS_FORESIGHT_CONTROL is set without SHEMS_FORESIGHT_HORIZON")
        return [], 1
    try:
        horizons = [int(x) for x in raw.split(",")]
    except ValueError:
        raise ValueError(f"SHEMS_FORESIGHT_HORIZON = {raw!r} is not an integer or a comma list of integers") from None
    if min(horizons) < 1:
        raise ValueError(f"SHEMS_FORESIGHT_HORIZON = {raw!r}: a plan sees at least the current hour")
    if control > min(horizons):
        raise ValueError(f"SHEMS_FORESIGHT_CONTROL = {control} exceeds a horizon of SHEMS_FORESIGHT_HORIZON = {raw!r}")
    return horizons, control


def foresight_regret(environ=os.environ):
    """SHEMS_FORESIGHT_REGRET=1 -> True: one <results file>_regret.csv next to every results file of the tracking block (the hourly
    regret against ONE perfect-foresight solve, harness.regret_of).  It needs SHEMS_FORESIGHT=1."""
    if environ.get("SHEMS_FORESIGHT_REGRET") != "1":
        return False
    if environ.get("SHEMS_FORESIGHT") != "1":
        raise ValueError("SHEMS_FORESIGHT_REGRET is set without SHEMS_FORESIGHT=1")
    return True


def foresight_imitate(environ=os.environ):
    """SHEMS_FORESIGHT_IMITATE=<rounds>x<steps> -> (rounds, steps), both >= 1: after the foresight pass a FRESH actor is trained by
    imitation of it (imitation.dagger: round 0 clones the foresight pass, every later round adds the audit's labels at the states the
    current actor visited), <steps> supervised updates per round; the per-round figures go to ..._results_<case>_imitation.csv beside
    the foresight file.  None when unset.  It needs SHEMS_FORESIGHT=1; a malformed value is refused by name."""
    raw = environ.get("SHEMS_FORESIGHT_IMITATE")
    if raw is None:
        return None
    if environ.get("SHEMS_FORESIGHT") != "1":
        raise ValueError("SHEMS_FORESIGHT_IMITATE is set without SHEMS_FORESIGHT=1")
    parts = raw.lower().split("x")
    try:
        rounds, steps = (int(x) for x in parts)
    except ValueError:
        raise ValueError(f"SHEMS_FORESIGHT_IMITATE = {raw!r} is not <rounds>x<steps>") from None
    if rounds < 1 or steps < 1:
        raise ValueError(f"SHEMS_FORESIGHT_IMITATE = {raw!r}: at least one round of at least one step")
    return rounds, steps


def foresight_warmstart(environ=os.environ):
    """SHEMS_FORESIGHT_WARMSTART=<critic_steps>[:td|:mc] -> (critic_steps >= 1, mode; "mc" when none is named): after the imitation
    block the SAME agent's critic is fitted by that many critic-only updates on the transitions of one pass of the cloned actor
    (imitation.warm_start); critic_loss_first and critic_loss_last go to ..._results_<case>_warmstart.csv beside the imitation file.
    None when unset.  It needs SHEMS_FORESIGHT_IMITATE; a malformed value is refused by name."""
    raw = environ.get("SHEMS_FORESIGHT_WARMSTART")
    if raw is None:
        return None
    if environ.get("SHEMS_FORESIGHT_IMITATE") is None:
        raise ValueError("SHEMS_FORESIGHT_WARMSTART is set without SHEMS_FORESIGHT_IMITATE")
    parts = raw.lower().split(":")
    try:
        steps = int(parts[0])
    except ValueError:
        steps = None
    if steps is None or len(parts) > 2 or (len(parts) == 2 and parts[1] not in ("td", "mc")):
        raise ValueError(f"SHEMS_FORESIGHT_WARMSTART = {raw!r} is not <critic_steps>[:td|:mc]")
    if steps < 1:
        raise ValueError(f"SHEMS_FORESIGHT_WARMSTART = {raw!r}: at least one critic step")
    return steps, parts[1] if len(parts) == 2 else "mc"


def bc_from_env(environ=os.environ):
    """SHEMS_BC=<alpha>[:<weight>] -> a ddpg.BC (the behaviour-regularised actor loss, normalised as the paper has it): the run trains with
    the term and `case` gains "_bc-a<alpha>-w<weight>" behind the other suffixes.  None when unset: today's bytes and names.  A malformed
    value is refused by name."""
    from .ddpg import parse_bc
    return parse_bc(environ.get("SHEMS_BC"))


def foresight_offline(environ=os.environ):
    """SHEMS_FORESIGHT_OFFLINE=<updates> -> updates >= 1: before the first episode the foresight pass of the TRAINING series goes into a
    "td" ring (imitation.transitions), the normalisation is set from that ring, and imitation.offline runs <updates> updates on it; the
    recorded rows go to ..._results_<case>_offline.csv beside the imitation file.  None when unset.  It needs SHEMS_FORESIGHT=1 and
    SHEMS_BC; a malformed value is refused by name."""
    raw = environ.get("SHEMS_FORESIGHT_OFFLINE")
    if raw is None:
        return None
    if environ.get("SHEMS_FORESIGHT") != "1":
        raise ValueError("SHEMS_FORESIGHT_OFFLINE is set without SHEMS_FORESIGHT=1")
    if environ.get("SHEMS_BC") is None:
        raise ValueError("SHEMS_FORESIGHT_OFFLINE is set without SHEMS_BC: offline training needs the behaviour-regularised actor loss")
    try:
        updates = int(raw)
    except ValueError:
        raise ValueError(f"SHEMS_FORESIGHT_OFFLINE = {raw!r} is not an integer number of updates") from None
    if updates < 1:
        raise ValueError(f"SHEMS_FORESIGHT_OFFLINE = {raw!r}: at least one update")
    return updates


def offline_file_name(job_id, run, case, out_dir="out/tracker"):
    """The recorded rows of SHEMS_FORESIGHT_OFFLINE, beside imitation_file_name's file."""
    return os.path.join(out_dir, f"{job_id}_{run}_results_{case}_offline.csv")


def warmstart_file_name(job_id, run, case, out_dir="out/tracker"):
    """The critic figures of SHEMS_FORESIGHT_WARMSTART, beside imitation_file_name's file."""
    return os.path.join(out_dir, f"{job_id}_{run}_results_{case}_warmstart.csv")


def imitation_file_name(job_id, run, case, out_dir="out/tracker"):
    """The per-round figures of SHEMS_FORESIGHT_IMITATE, beside harness.foresight_file_name's file."""
    return os.path.join(out_dir, f"{job_id}_{run}_results_{case}_imitation.csv")


def foresight_forecast(environ=os.environ):
    """SHEMS_FORESIGHT_FORECAST = persistence[:LAG[:ev]] -> (lag, ev), or analog:LAG,LAG,...[:ev] -> ("analog", (lags), ev) (1 .. 16
    lags, each >= 1); None when unset.  It needs SHEMS_FORESIGHT_HORIZON; a malformed value is refused by name."""
    raw = environ.get("SHEMS_FORESIGHT_FORECAST")
    if raw is None:
        return None
    if environ.get("SHEMS_FORESIGHT_HORIZON") is None:
        raise ValueError("SHEMS_FORESIGHT_FORECAST is set without SHEMS_FORESIGHT_HORIZON")
    parts = raw.split(":")
    if parts[0] == "analog":
        if len(parts) not in (2, 3) or (len(parts) == 3 and parts[2] != "ev"):
            raise ValueError(f"SHEMS_FORESIGHT_FORECAST = {raw!r} is not analog:LAG,LAG,...[:ev]")
        try:
            lags = tuple(int(x) for x in parts[1].split(","))
        except ValueError:
            raise ValueError(f"SHEMS_FORESIGHT_FORECAST = {raw!r}: the lags are not a comma list of integers") from None
        if min(lags) < 1 or len(lags) > 16:
            raise ValueError(f"SHEMS_FORESIGHT_FORECAST = {raw!r}: 1 .. 16 lags of 1 or more hours each")
        return "analog", lags, len(parts) == 3
    if parts[0] != "persistence" or len(parts) > 3 or (len(parts) == 3 and parts[2] != "ev"):
        raise ValueError(f"SHEMS_FORESIGHT_FORECAST = {raw!r} is not persistence[:LAG[:ev]]")
    try:
        lag = 24 if len(parts) == 1 else int(parts[1])
    except ValueError:
        raise ValueError(f"SHEMS_FORESIGHT_FORECAST = {raw!r}: LAG is not an integer") from None
    if lag < 1:
        raise ValueError(f"SHEMS_FORESIGHT_FORECAST = {raw!r}: a lag of 1 or more hours")
    return lag, len(parts) == 3


def _check_supported(cfg):
    # (250, 500): the tuned kernels; smaller: zero-padded into them (ddpg.pad_net); larger -- the grids' (300, 600) --: the layer-by-layer
    # wide path (csrc/shems_wide.hip, ddpg.is_wide)
    if not (1 <= cfg.L1 <= 4096 and 1 <= cfg.L2 <= 4096):
        raise NotImplementedError(f"JOB_ID {cfg.job_id} selects (L1, L2) = ({cfg.L1}, {cfg.L2})")
    if not 1 <= cfg.BATCH_SIZE <= 1024:             # above 128: replay() runs the gradient passes per sub-batch (ddpg.Agent._replay_wide)
        raise NotImplementedError(f"JOB_ID {cfg.job_id} selects BATCH_SIZE = {cfg.BATCH_SIZE}")
    if cfg.noise_type not in ("gn", "ou", "en", "pn"):
        raise NotImplementedError(f"JOB_ID {cfg.job_id} selects noise_type = {cfg.noise_type!r} (DDPG.jl:152-161 knows gn, ou, en, pn)")
    if cfg.noise_type == "pn":
        # parameter noise adds one scalar to EVERY parameter (DDPG.jl:89-96): it would un-zero the padding a smaller network runs with,
        # and its adaptation step reads the minibatch of ONE update pass (128 columns) -- refuse here, before populate_memory, not at the
        # first replay()
        from .ddpg import L1 as _L1, L2 as _L2, is_wide
        if (cfg.L1, cfg.L2) != (_L1, _L2) and not is_wide((cfg.L1, cfg.L2)):
            raise NotImplementedError(f"JOB_ID {cfg.job_id} selects parameter noise with (L1, L2) = ({cfg.L1}, {cfg.L2}): a network smaller than "
                                      f"({_L1}, {_L2}) runs zero-padded, which parameter noise would break")
        if cfg.BATCH_SIZE > 128:
            raise NotImplementedError(f"JOB_ID {cfg.job_id} selects parameter noise with BATCH_SIZE = {cfg.BATCH_SIZE} > 128 (adapt_param_noise! on sub-batches)")


def data_path(cfg, split, data_dir="data", charger=None):
    return os.path.join(data_dir, f"{charger or cfg.Charger_ID}_{cfg.season}_{split}_{cfg.price}.csv")      # INPUT:162-164


def main(environ=os.environ, cwd=".", log=print):
    import torch
    from . import checkpoint, harness, tables
    from . import ddpg as D
    from .env import ShemsBatch, make_config

    cfg = config_from_env(environ)
    _check_supported(cfg)
    algo, td3_hp = algo_from_env(environ)
    if algo == "td3":
        from . import td3 as T
        if cfg.L1 > 250 or cfg.L2 > 500 or cfg.BATCH_SIZE > 128 or cfg.noise_type == "pn":
            raise ValueError(f"SHEMS_ALGO=td3: the twin-critic update holds networks up to (250, 500), batches up to 128 and no parameter "
                             f"noise, not ({cfg.L1}, {cfg.L2}) at {cfg.BATCH_SIZE} with noise_type = {cfg.noise_type!r}")
        cfg.algo_suffix = T.case_suffix(**td3_hp)
    replay_kind, per_hp = replay_from_env(environ)
    if replay_kind == "per":
        if algo == "td3":
            raise NotImplementedError("SHEMS_REPLAY=per with SHEMS_ALGO=td3: the twin-critic update has no weighted head")
        if cfg.L1 > 250 or cfg.L2 > 500 or cfg.BATCH_SIZE > 128 or cfg.noise_type == "pn":
            raise ValueError(f"SHEMS_REPLAY=per: the prioritized update holds networks up to (250, 500), batches up to 128 and no parameter "
                             f"noise, not ({cfg.L1}, {cfg.L2}) at {cfg.BATCH_SIZE} with noise_type = {cfg.noise_type!r}")
        cfg.algo_suffix += replay_case_suffix(**per_hp)
    n_step = nstep_from_env(environ)
    cfg.algo_suffix += nstep_case_suffix(n_step)
    if n_step > 1 and environ.get("SHEMS_FORESIGHT_WARMSTART") is not None:
        raise NotImplementedError(f"SHEMS_NSTEP = {n_step} with SHEMS_FORESIGHT_WARMSTART: the warm start seeds the ring with one-step "
                                  "transitions, which an n-step learner would bootstrap with gamma^n")
    if n_step > EP_LENGTH["train"]:
        raise ValueError(f"SHEMS_NSTEP = {n_step}: a training episode of {EP_LENGTH['train']} hours holds no full window")
    bc = bc_from_env(environ)
    if bc is not None:
        if replay_kind == "per":
            raise NotImplementedError("SHEMS_BC with SHEMS_REPLAY=per: the weighted update has no behaviour-regularised head")
        if cfg.L1 > 250 or cfg.L2 > 500 or cfg.BATCH_SIZE > 128 or cfg.noise_type == "pn":
            raise ValueError(f"SHEMS_BC: the behaviour-regularised update holds networks up to (250, 500), batches up to 128 and no parameter "
                             f"noise, not ({cfg.L1}, {cfg.L2}) at {cfg.BATCH_SIZE} with noise_type = {cfg.noise_type!r}")
        cfg.algo_suffix += D.bc_case_suffix(bc)
    offline = foresight_offline(environ)
    horizons, control = foresight_horizons(environ) if environ.get("SHEMS_FORESIGHT") == "1" else ([], 1)
    forecast = foresight_forecast(environ) if environ.get("SHEMS_FORESIGHT") == "1" else None
    regret = foresight_regret(environ)
    imitate = foresight_imitate(environ)
    warmstart = foresight_warmstart(environ)
    if imitate is not None and replay_kind == "per":
        raise NotImplementedError("SHEMS_REPLAY=per with SHEMS_FORESIGHT_IMITATE: the supervised and critic-only updates draw uniformly")
    if imitate is not None and (cfg.L1 > 250 or cfg.L2 > 500 or cfg.BATCH_SIZE > 128):
        raise ValueError(f"SHEMS_FORESIGHT_IMITATE: the supervised update holds networks up to (250, 500) and batches up to 128, not "
                         f"({cfg.L1}, {cfg.L2}) at {cfg.BATCH_SIZE}")
    os.chdir(cwd)
    torch.cuda.set_device(cfg.gpu_id)                                    # CUDA.device!(gpu_id), MAIN:12-14
    if cfg.seed_run == 1:
        log(f"Using bash scheduler.\n\tMax steps: {EP_LENGTH['train']} | Max episodes: {cfg.NUM_EP} | Layer 1: {cfg.L1} nodes | "
            f"Layer 2: {cfg.L2} nodes |\n\tCase: {cfg.case}")
    log(f"Starting script with JOB_ID: {cfg.job_id}, TASK_ID: {cfg.task_id} for charger {cfg.Charger_ID} on GPU: {cfg.gpu_id}!")

    if environ.get("SHEMS_SYNTHETIC_DATA") == "1":                       # demo / tests: the per-charger CSVs are not public (README.md:12)
        os.makedirs("data", exist_ok=True)
        for split in ("train", "eval", "test"):
            p = data_path(cfg, split)
            if not os.path.exists(p):
                t = tables.profile_table(cfg.charger_id, split)
                need = 1 + (EP_LENGTH["train"] if split == "train" else EP_LENGTH[cfg.season, split])    # a pass of n steps reads row n + 1
                if t.shape[0] < need:                                      # a real series with one row per MPC decision: see tables.pad_rows
                    log(f"{os.path.basename(p)}: {t.shape[0]} rows in the reconstructed series, {need} needed; padded with the rows 24 h earlier")
                    t = tables.pad_rows(t, need)
                tables.save_csv(p, t)
    tabs = {split: tables.load_csv(data_path(cfg, split)) for split in ("train", "eval", "test")}       # env_dict, INPUT:162-164
    n_envs = int(environ.get("SHEMS_NUM_ENVS", "1"))
    # the env's reward weights are module constants of shems_LU1.jl:40-43 (0.01f0, 2f0, 0.1f0) whatever the input file says ("REMEMBER TO
    # ADJUST THIS IN ENV", INPUT:80-81): the input's values only enter the `case` string
    mk = lambda n, steps, tab: ShemsBatch(n, steps, [tab], [make_config(cfg.charger_id, 0, tab.shape[0])], device=cfg.gpu_id).use_torch_stream()
    env_train = mk(n_envs, EP_LENGTH["train"], tabs["train"])
    env_eval = mk(cfg.test_runs, EP_LENGTH[cfg.season, "eval"], tabs["eval"])
    env_track = mk(1, EP_LENGTH[cfg.season, cfg.run], tabs[cfg.run])

    D.GAMMA, D.TAU = cfg.gamma, cfg.tau
    if algo == "td3":
        agent = T.TD3Agent(seed=cfg.rng_run, sigma=cfg.noise_act if cfg.noise_type == "gn" else cfg.sigma, noise_type=cfg.noise_type,
                           theta=cfg.theta, hidden=(cfg.L1, cfg.L2), n_step=n_step, bc=bc, **td3_hp)
    else:
        agent = D.Agent(seed=cfg.rng_run, sigma=cfg.noise_act if cfg.noise_type == "gn" else cfg.sigma, noise_type=cfg.noise_type,
                        theta=cfg.theta, hidden=(cfg.L1, cfg.L2), n_step=n_step, bc=bc)
    agent.gamma, agent.tau, agent.batch = float(np.float32(cfg.gamma)), float(np.float32(cfg.tau)), cfg.BATCH_SIZE
    agent.eta_act, agent.eta_crit = float(np.float32(cfg.eta_act)), float(np.float32(cfg.eta_crit))
    ring = D.PrioritizedRing(cfg.MEM_SIZE, alpha=per_hp["alpha"], beta=per_hp["beta0"]) if replay_kind == "per" else D.ReplayRing(cfg.MEM_SIZE)
    ck = dict(ep_len=EP_LENGTH["train"], num_ep=cfg.NUM_EP, l1=cfg.L1, l2=cfg.L2, case=cfg.case)

    # ---- Memory Buffer (MAIN:27-30) ----
    agent.populate_memory(env_train, ring, seed=cfg.rng_run)
    offline_written = []
    if offline is None:
        agent.min_max_buffer(ring, cfg.MEM_SIZE, seed=cfg.rng_run)
    else:                                                                # offline training on the foresight pass of the training series
        from . import imitation
        steps = tabs["train"].shape[0] - 1                               # (a pass of n steps reads row n + 1)
        env_off = mk(1, steps, tabs["train"])
        values = harness.foresight_values(env_off)
        _, res_off = harness.inference_foresight(env_off, values=values)
        seeded = D.ReplayRing(steps)
        imitation.transitions(values, res_off[0], seeded, mode="td", gamma=agent.gamma)
        agent.min_max_buffer(seeded, len(seeded), seed=cfg.rng_run)      # the normalisation of the run: the training below keeps it
        rows = imitation.offline(agent, seeded, offline, record_every=max(1, offline // 100))
        offline_written.append(imitation.write_to_offline_file(rows, offline_file_name(cfg.job_id, cfg.run, cfg.case)))
        env_off.close()
        log(f"offline: {offline} updates on {len(seeded)} transitions of the foresight pass; mse(a_pi, a) {rows[0][4]:.4g} -> {rows[-1][4]:.4g}")

    noise_mean = np.zeros(cfg.NUM_EP, np.float32)
    best_eval = 0
    if cfg.train:
        t0 = time.time()
        log(f", Training run: {cfg.rng_run}")

        def on_best(i, actor, total_reward, score_mean):                 # saveBSON(...; idx=i, path="temp", rng=rng_run), DDPG.jl:282-286
            checkpoint.save(actor, total_reward, score_mean, i, agent.noise_mean, idx=i, rng=cfg.rng_run, path="temp", **ck)

        total_reward, score_mean, best_eval, _ = agent.run_episodes(env_train, env_eval, ring, cfg.NUM_EP, test_every=cfg.test_every,
                                                                    test_runs=cfg.test_runs, seed=cfg.rng_run, on_best=on_best,
                                                                    **(dict(anneal_beta_from=per_hp["beta0"]) if replay_kind == "per" else {}))
        noise_mean = agent.noise_mean
        checkpoint.save(agent.export_actor(), total_reward, score_mean, best_eval, noise_mean, idx=cfg.NUM_EP, rng=cfg.rng_run, **ck)   # MAIN:45-46
        log(f"trained {cfg.NUM_EP} episodes in {time.time() - t0:.1f} s; best evaluation at episode {best_eval}")

    # ---- track evaluation (MAIN:87-110) ----
    written, audited = list(offline_written), []                         # audited: (results path, rows) of every pass stepped on the true table
    tk = dict(num_ep=cfg.NUM_EP, l1=cfg.L1, l2=cfg.L2, batch_size=cfg.BATCH_SIZE, mem_size=cfg.MEM_SIZE, min_exp_size=cfg.MEM_SIZE,
              season=cfg.season, run=cfg.run, job_id=cfg.job_id, case=cfg.case)
    if cfg.track == 1 and cfg.seed_run == cfg.num_seeds:
        log(f"Evaluation/Testing for TASK_IDs of {cfg.job_id}.")
        # every seed's last and best actor (MAIN:90-103) -> ONE launch: pass p of the batch runs the whole data set with actor p
        # (harness.inference_many / shems_track_dev); the files are then written in the reference's order.  s_min / s_max are this
        # process's, as in the reference (module globals of the evaluating task).
        passes = []                                                      # (test_rng_run, best, idx, actor)
        for i in range(1, cfg.num_seeds + 1):
            test_rng_run = int(str(SEED_INI) + str(i))
            try:
                ac, _, _, best_i, _ = checkpoint.load(idx=cfg.NUM_EP, rng=test_rng_run, **ck)
            except FileNotFoundError:
                log(f"  seed {i}: no snapshot of run {test_rng_run} (that task has not finished): skipped")
                continue
            passes.append((test_rng_run, False, cfg.NUM_EP, ac))
            passes.append((test_rng_run, True, best_i, checkpoint.load(idx=best_i, rng=test_rng_run, path="temp", **ck)[0]))
        if passes:
            env_many = mk(len(passes), EP_LENGTH[cfg.season, cfg.run], tabs[cfg.run])
            hid = (cfg.L1, cfg.L2)                                       # checkpoints hold the network's own size: pad into the kernels' layout
            lay = (lambda a: np.asarray(a, np.float32)) if D.is_wide(hid) else (lambda a: D.pad_net(a, 9, 2, hid))      # (a wide one keeps its own)
            _, results = harness.inference_many(env_many, np.stack([lay(p[3]) for p in passes]), agent.s_min, agent.s_max, hidden=hid)
            env_many.close()
            for (test_rng_run, best, idx, _), res in zip(passes, results):
                path = harness.results_file_name(cfg.job_id, cfg.run, EP_LENGTH["train"], cfg.NUM_EP, cfg.L1, cfg.L2, cfg.case, test_rng_run,
                                                 cfg.NUM_EP, best=best)
                harness.write_to_results_file(res, path)
                harness.write_to_tracker_file(path, seed=test_rng_run, best=best, idx=idx, **tk)
                written.append(path)
                audited.append((path, res))
        log(f"Evaluation/Testing for TASK_IDs of {cfg.job_id} is finished.")
    elif cfg.track < 0:                                                  # rule-based
        _, results = harness.inference(env_track, None, track=cfg.track)
        idx = cfg.track if cfg.track != int(cfg.track) else int(cfg.track)
        path = harness.results_file_name(cfg.job_id, cfg.run, EP_LENGTH["train"], cfg.NUM_EP, cfg.L1, cfg.L2, cfg.case, cfg.track, idx)
        harness.write_to_results_file(results, path)
        harness.write_to_tracker_file(path, seed=idx, best=False, idx=idx, **tk)
        written.append(path)
        audited.append((path, results))
    if environ.get("SHEMS_FORESIGHT") == "1":                            # this build's addition: the upper yardstick on the same table
        values = harness.foresight_values(env_track) if regret or imitate is not None else None   # the one perfect-foresight solve every audit below reads
        _, results = harness.inference_foresight(env_track, values=values)
        path = harness.foresight_file_name(cfg.job_id, cfg.run, cfg.case)
        harness.write_to_results_file(results[0], path)
        harness.write_to_tracker_file(path, seed="foresight", best=False, idx=0, **tk)
        written.append(path)
        audited.append((path, results[0]))
        env_fc = None
        fc_kw = {}
        if forecast is not None:                                         # the same table with its persistence forecast(s) behind it
            from . import foresight
            cols = ("electkwh", "PV_generation") + (foresight.EV_COLUMNS if forecast[-1] else ())
            if forecast[0] == "analog":                                  # the ensemble: one scenario table per lag, equal weights
                both, sc_index = foresight.append_scenarios([tabs[cfg.run]], forecast[1], cols)
                fc_kw = dict(scenario_tables=sc_index[0])
            else:
                both, fc_index = foresight.append_forecasts([tabs[cfg.run]], forecast[0], cols)
                fc_kw = dict(forecast_table=fc_index[0])
            env_fc = ShemsBatch(1, EP_LENGTH[cfg.season, cfg.run], both, [make_config(cfg.charger_id, 0, tabs[cfg.run].shape[0])],
                                device=cfg.gpu_id).use_torch_stream()
        for h in horizons:                                               # the deployable case: h hours of forecast, a plan every `control`
            _, results = harness.inference_foresight(env_track, horizon=h, control=control)
            path = harness.foresight_file_name(cfg.job_id, cfg.run, cfg.case, horizon=h, control=control)
            harness.write_to_results_file(results[0], path)
            harness.write_to_tracker_file(path, seed=harness.foresight_seed(h, control), best=False, idx=0, **tk)
            written.append(path)
            audited.append((path, results[0]))
            if env_fc is not None:                                       # ... and planning on a forecast that is wrong
                _, results = harness.inference_foresight(env_fc, horizon=h, control=control, **fc_kw)
                path = harness.foresight_file_name(cfg.job_id, cfg.run, cfg.case, horizon=h, control=control, forecast=forecast)
                harness.write_to_results_file(results[0], path)
                harness.write_to_tracker_file(path, seed=harness.foresight_seed(h, control, forecast), best=False, idx=0, **tk)
                written.append(path)
                audited.append((path, results[0]))                       # stepped on the truth: audited against the truth, not its belief
        if env_fc is not None:
            env_fc.close()
        if regret:                                                       # all passes in one launch against the one solve
            audit = harness.regret_of(env_track, np.stack([r for _, r in audited]), values=values)
            for k, (path, res) in enumerate(audited):
                written.append(harness.write_to_regret_file(audit, res, harness.regret_file_name(path), pass_index=k))
        if imitate is not None:                                          # a fresh actor trained by imitation of the foresight pass
            from . import imitation
            pupil = D.Agent(seed=cfg.rng_run, hidden=(cfg.L1, cfg.L2))
            pupil.batch, pupil.eta_act = cfg.BATCH_SIZE, float(np.float32(cfg.eta_act))
            demos = imitation.Demos(imitate[0] * EP_LENGTH[cfg.season, cfg.run])
            if warmstart is None:
                figures = imitation.dagger(pupil, env_track, values, demos, imitate[0], imitate[1])
            else:                                                        # the same agent's critic fitted on a pass of the cloned actor
                pupil.gamma, pupil.tau = float(np.float32(cfg.gamma)), float(np.float32(cfg.tau))
                pupil.eta_crit = float(np.float32(cfg.eta_crit))
                fitted = D.ReplayRing(EP_LENGTH[cfg.season, cfg.run])
                *figures, critic = imitation.warm_start(pupil, env_track, values, demos, fitted, imitate[0], imitate[1], warmstart[0],
                                                        mode=warmstart[1])
            written.append(imitation.write_to_imitation_file(figures, imitation_file_name(cfg.job_id, cfg.run, cfg.case)))
            if warmstart is not None:
                written.append(imitation.write_to_warmstart_file(critic, warmstart_file_name(cfg.job_id, cfg.run, cfg.case)))
    for e in (env_train, env_eval, env_track):
        e.close()
    log(f"Script with JOB_ID: {cfg.job_id} & TASK_ID: {cfg.task_id} is done!")
    return cfg, written


if __name__ == "__main__":
    main()
