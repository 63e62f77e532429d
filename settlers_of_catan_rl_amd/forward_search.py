"""Batched forward search (reference RL/forward_search_policy/*; BASELINE.json configs[4]).

The reference planner decides ONE move of ONE game: it proposes <= 10 root actions with the policy
(`default_sample_actions`, sample_actions_fn.py:55-328), then for a wall-clock budget lets 11 CPU worker processes run
simulations - restore the root state, `randomise_uncertainty`, play the proposed action, then up to `max_depth` further
decisions of the searching player with the policy acting for every seat, and score the line with a GAE-style estimate
(worker.py:39-143) - allocating simulations to root actions with a UCB rule (policy.py:151-177).

Here R root games are searched at once.  Every piece keeps the reference's arithmetic and quirks:
  * `propose_actions`  - default_sample_actions for all roots: one batched, type-conditioned policy call per step of the
                         procedure (13 first-pass types + <= max_actions refinement draws) instead of one call per root.
  * `simulate`         - run_simulation_forward for n simulations in lock-step on a VecCatanEnv (dense rewards, no
                         auto-reset): incl. the simulator's get_players_turn that ignores the discard phase and the
                         `elif done` reward rule.
  * `gae_estimate`     - worker.gae, vectorised over simulations (the unused final value, the `len(values) <= 1` shortcut).
  * `UCBStats`         - _select_action / _update_stats / MovingAvgCalculator, vectorised over roots (host, float64).
  * `ForwardSearch`    - the act() loop in rounds of K simulations per root (inside a round simulations are allocated one
                         after the other exactly as the reference hands them to free workers), with a fixed simulation
                         budget (the reference's own "deterministic testing" variant, policy.py:112) or the reference's
                         wall-clock budget per root (`max_thinking_time`, policy.py:91,111); LSTM policies carry every
                         seat's (h, c) through proposals and simulations (policy.py:72-106, worker.py:61-95).
State broadcast = catan_state_fork (records copied on the device) or catan_state_export / catan_state_import; every simulation
gets its own Philox substream.
"""
import math
import random as _py_random

import numpy as np
import torch

from . import acting, spec
from .acting import GraphedAct     # (the name tools and tests import from here)

MAX_PROP_TRADE_ACTIONS = 3                                   # sample_actions_fn.py:6
PRIORITIES = [["settlement", "city", "move_robber", "steal", "discard"], ["road"], ["play_dev"], ["exchange_res", "prop_trade"]]
TYPE_TO_IND = {"settlement": 0, "road": 1, "city": 2, "buy_dev": 3, "play_dev": 4, "exchange_res": 5, "prop_trade": 6,
               "respond_trade": 7, "move_robber": 8, "roll_dice": 9, "end_turn": 10, "steal": 11, "discard": 12}
MO = spec.MASK_OFFSETS
# "fork" may become the default only once tools/bench_state_fork.py has shown catan_state_fork not slower than the per-round blob
# path on an MI355X (profiles/state_fork_bench.txt); that file does not exist yet, so the default is the path that was there before
DEFAULT_STATE_BROADCAST = "blob"


# ---------------------------------------------------------------------------------------------------- worker.gae
def gae_estimate(values, n_values, rewards, n_rewards, gamma, done, gae_lambda=0.95):
    """worker.py:117-143 for a batch: values [n, *] / rewards [n, *] hold n_values[i] / n_rewards[i] valid entries.
    -> float64 [n]."""
    values = np.asarray(values, dtype=np.float64); rewards = np.asarray(rewards, dtype=np.float64)
    n_values = np.asarray(n_values); n_rewards = np.asarray(n_rewards); done = np.asarray(done, dtype=bool)
    n = values.shape[0]
    out = np.zeros(n, dtype=np.float64)
    short = n_values <= 1                                     # `return rewards[0] + gamma * rewards[1]`
    if short.any():
        assert (n_rewards[short] >= 2).all(), "worker.gae indexes rewards[1] here (IndexError in the reference)"
        out[short] = rewards[short, 0] + gamma * rewards[short, 1]
    idx = np.flatnonzero(~short)
    if idx.size:
        v = values[idx]; r = rewards[idx]; nv = n_values[idx]; d = done[idx]
        num_steps = nv - 2                                    # len(values[:-1]) - 1
        g = np.zeros(idx.size, dtype=np.float64)
        for step in range(int(num_steps.max()) - 1, -1, -1):
            live = step < num_steps
            delta = r[:, 1 + step] + gamma * v[:, step + 1] - v[:, step]      # rewards_for_gae = rewards[1:-1]
            last = live & (step == num_steps - 1) & d
            g = np.where(last, delta, np.where(live, delta + gamma * gae_lambda * g, g))
        out[idx] = r[:, 0] + gamma * (g + v[:, 0])
    return out


# ---------------------------------------------------------------------------------------------------- UCB bookkeeping
class UCBStats(object):
    """policy.py:151-177 + utils.MovingAvgCalculator for R roots; root i has n_actions[i] proposed actions."""
    PERSISTENT = ("window", "num_added", "avg", "var", "last_std")      # the moving average: what outlives a decision

    def __init__(self, n_roots, max_actions, window=500):
        R, A = n_roots, max_actions
        self.R, self.A = R, A
        self.window = np.zeros((R, window)); self.window_size = window
        self.num_added = np.zeros(R, dtype=np.int64)
        self.avg = np.zeros(R); self.var = np.zeros(R); self.last_std = np.zeros(R)
        self.new_decision(np.zeros(R, dtype=np.int64))

    def new_decision(self, n_actions):
        """act(): the per-decision counters restart, the value moving average persists (policy.py:48,96-100)."""
        self.n_actions = np.asarray(n_actions)
        self.finished = np.zeros(self.R, dtype=np.int64)
        self.finished_each = np.zeros((self.R, self.A)); self.started_each = np.zeros((self.R, self.A))
        self.exploit = np.zeros((self.R, self.A))

    def grow(self, n_roots):
        """rows for roots up to n_roots - 1 (new ones start with an empty window)"""
        if n_roots <= self.R:
            return
        new = UCBStats(n_roots - self.R, self.A, self.window_size)
        for k in self.PERSISTENT:
            setattr(self, k, np.concatenate((getattr(self, k), getattr(new, k))))
        self.R = n_roots
        self.new_decision(np.zeros(n_roots, dtype=np.int64))

    def take(self, rows):
        """-> the bookkeeping of the roots `rows` alone (copies), for one decision of theirs; `put` stores their moving averages back"""
        sub = UCBStats(len(rows), self.A, self.window_size)
        for k in self.PERSISTENT:
            setattr(sub, k, getattr(self, k)[rows].copy())
        return sub

    def put(self, rows, sub):
        for k in self.PERSISTENT:
            getattr(self, k)[rows] = getattr(sub, k)

    def select(self, explore=True):
        """_select_action for every root (first best index wins ties, `score > best_score`)."""
        exploit = self.exploit / (self.finished_each + 1e-5)
        score = exploit
        if explore:
            explore_score = np.sqrt(2.0 * np.log(self.finished + 2)[:, None] / (self.finished_each + self.started_each + 1e-10))
            score = exploit + 2.0 * np.maximum(self.last_std, 1.0)[:, None] * explore_score
        score = np.where(np.arange(self.A)[None, :] < self.n_actions[:, None], score, -np.inf)
        return np.argmax(score, axis=1)

    def start(self, action_id, sel=None):
        """action_id: one id per root (all R); sel: the roots that really start the simulation"""
        rows = np.arange(self.R) if sel is None else np.asarray(sel)
        self.started_each[rows, np.asarray(action_id)[rows] if sel is not None else action_id] += 1

    def update(self, val, action_id, sel=None):
        """_update_stats + MovingAvgCalculator.update for one finished simulation per selected root."""
        rows = np.arange(self.R) if sel is None else np.asarray(sel)
        val = np.asarray(val, dtype=np.float64)
        self.started_each[rows, action_id] -= 1
        self.finished[rows] += 1
        self.finished_each[rows, action_id] += 1
        self.exploit[rows, action_id] += val
        # utils.py:14-46
        k = self.num_added[rows] % self.window_size
        old_value = self.window[rows, k]
        self.window[rows, k] = val
        self.num_added[rows] += 1
        na = self.num_added[rows]
        old_avg = self.avg[rows].copy()
        filling = na <= self.window_size
        delta = np.where(filling, val - old_avg, val - old_value)
        avg = old_avg + np.where(filling, delta / na, delta / self.window_size)
        var = self.var[rows] + np.where(filling, delta * (val - avg), delta * ((val - avg) + (old_value - old_avg)))
        self.avg[rows] = avg; self.var[rows] = var
        variance = np.where(filling, np.where(na == 1, 1.0, var / np.maximum(na - 1, 1)), var / self.window_size)
        with np.errstate(invalid="ignore"):
            std = np.sqrt(variance)
        self.last_std[rows] = np.where(np.isnan(std), 0.1, std)       # `except: std = 0.1` / isnan


# ---------------------------------------------------------------------------------------------------- simulations
@torch.no_grad()
def simulate(env, policy, ctrl, init_actions, max_depth=20, gamma=0.999, deterministic=False, generator=None, autocast_dtype=None,
             graphed=None, hidden=None, init_hidden=None, idle=None):
    """run_simulation_forward (worker.py:61-114) for all env.n simulations in lock-step.  idle (bool [n], optional): rows that hold no
    simulation - they take no step (action type -1 throughout), are in no policy pass, and their entry of the result means nothing.  env: dense-reward, no auto-reset,
    already holding the (randomised) start states; ctrl int [n] PlayerId of the searching player; init_actions [n,18].
    LSTM policies (`include_lstm`): hidden [2, n, 4, L] = every seat's (h, c) at the start state (`curr_hidden_states`),
    init_hidden [2, n, L] = the searching seat's state after it took the initial action (`init_player_hs`, worker.py:73); each
    decision runs from the deciding seat's state and stores the new one (:84-95; the terminal mask is 1 throughout).
    -> float64 numpy [n] value estimates."""
    n, dev = env.n, env.device
    ar = torch.arange(n, device=dev)
    ctrl = torch.as_tensor(ctrl, device=dev).long()
    D = max_depth
    rewards = torch.zeros((n, D + 2), dtype=torch.float64, device=dev); n_rew = torch.zeros(n, dtype=torch.long, device=dev)
    values = torch.zeros((n, D + 1), dtype=torch.float64, device=dev); n_val = torch.zeros(n, dtype=torch.long, device=dev)

    def push(buf, cnt, sel, x):                         # append x[i] to row i's list where sel[i] (masked write: no host read)
        c = cnt.clamp(max=buf.shape[1] - 1)
        buf[ar, c] = torch.where(sel, x.double(), buf[ar, c])
        cnt += sel.long()

    a0 = torch.as_tensor(init_actions, device=dev).to(torch.int32)
    if idle is not None:
        idle = torch.as_tensor(idle, device=dev).bool()
        a0 = a0.clone()
        a0[:, 0] = torch.where(idle, torch.full_like(a0[:, 0], -1), a0[:, 0])
    reward, done = env.step(a0)                                                             # worker.py:71
    reward = reward.clone(); first_done = done.bool().clone()
    if idle is not None:
        first_done |= idle                                                                  # nothing to estimate for them
    push(rewards, n_rew, torch.ones(n, dtype=torch.bool, device=dev), reward[ar, ctrl - 1])
    agent_actions = torch.ones(n, dtype=torch.long, device=dev)
    active = ~first_done                                                                    # `if done: return actual_rewards[0]`
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    rec = bool(getattr(policy, "include_lstm", False))
    if rec:
        L = int(policy.lstm_size)
        hid = torch.zeros((2, n, 4, L), dtype=torch.float32, device=dev) if hidden is None else hidden.to(dev).float().clone()
        if init_hidden is not None:
            hid[:, ar, ctrl - 1] = init_hidden.to(dev).float()                              # worker.py:73
        graphed = None
    # (device env with the game-list views: see the loop)
    lists_of_games = (not rec) and hasattr(env, "get_obs_rows") and hasattr(env, "L") and getattr(env, "device", None) is not None and torch.device(env.device).type == "cuda"
    while True:
        live = active & (agent_actions < D)                                                 # worker.py:81
        if not bool(live.any()):
            break
        players_go = env.players_turn_sim().long()                                          # :82, 146-151
        # only the simulations still running need a decision (the batch thins out as lines reach max_depth or end)
        idx = live.nonzero(as_tuple=True)[0]
        sub = idx.numel() < n
        if lists_of_games and graphed is not None and idx.numel() <= graphed.buckets[-1]:
            # the observations and masks of the LIVE games only, straight into the captured pass's input buffers (catan_obs_rows_of /
            # catan_masks_of; bf16 under bf16 autocast: every value is a multiple of 1/8): all games' fp32 observations + a gather of
            # the live rows + the net's cast + the copy into the graph's buffers were 15 % of a batch of root decisions
            games = idx.to(torch.int32)
            nl = int(idx.numel())
            odt = autocast_dtype if autocast_dtype in (torch.bfloat16,) else torch.float32
            bufs = graphed.input_rows(next(b for b in graphed.buckets if nl <= b), nl, odt)
            f, lists, lens = env.get_obs_rows(odt, out=None if bufs is None else bufs[:3], games=games)
            masks = env.get_action_masks(None if bufs is None else bufs[3], games=games)
            args = (f, lists, lens, masks)
        else:
            f, lists, lens = env.get_obs()
            masks = env.get_action_masks()
            args = (f[idx], lists[idx], lens[idx].long(), masks[idx]) if sub else (f, lists, lens.long(), masks)
        kw = {}
        if rec:
            seat = players_go[idx] - 1
            kw = {"hidden": (hid[0, idx, seat], hid[1, idx, seat]), "nonterminal": torch.ones(idx.numel(), device=dev)}
        if graphed is not None and idx.numel() <= graphed.buckets[-1]:
            value_s, action_s = graphed(*args)                                             # hipGraph replay of the pass at the next bucket size (a pass is launch-bound at every width up to 65 536 rows)
        else:
            res = acting.act(policy, args, autocast_dtype, deterministic=deterministic, generator=generator, **kw)
            value_s, action_s = res[0], res[1]
        if rec:
            hid[0, idx, seat], hid[1, idx, seat] = res[3][0].float(), res[3][1].float()     # :95
        if sub:
            value = torch.zeros((n, 1), dtype=value_s.dtype, device=dev); value[idx] = value_s
            action = torch.zeros((n, spec.ACTION_WORDS), dtype=action_s.dtype, device=dev); action[idx] = action_s
        else:
            value, action = value_s, action_s
        value = policy.denormalise(value.float()[:, 0])                                     # :92-93
        a_env = action.to(torch.int32)
        a_env[:, 0] = torch.where(live, a_env[:, 0], torch.full_like(a_env[:, 0], -1))     # finished simulations idle
        reward, done = env.step(a_env)
        done = done.bool() & live
        r_ctrl = reward[ar, ctrl - 1]
        is_agent = live & (players_go == ctrl)                                              # :99-104
        agent_actions += is_agent.long()
        push(rewards, n_rew, is_agent | (live & ~is_agent & done), r_ctrl)
        push(values, n_val, is_agent, value)
        finished |= done                                                                    # :109-111
        active &= ~done
    fd = first_done.cpu().numpy()
    rewards_h = rewards.cpu().numpy()
    out = rewards_h[:, 0].copy()                                                            # `if done: return actual_rewards[0]`
    rest = np.flatnonzero(~fd)
    if rest.size:
        out[rest] = gae_estimate(values.cpu().numpy()[rest], n_val.cpu().numpy()[rest], rewards_h[rest], n_rew.cpu().numpy()[rest],
                                 gamma, finished.cpu().numpy()[rest])
    return out


# ---------------------------------------------------------------------------------------------------- proposals
def _update_action_masks(action, m):
    """sample_actions_fn.py:31-53 on one flat mask row (numpy float [325]) - removes the proposed target from its head."""
    t = int(action[0])
    if t == 0:
        if m[MO[1]:MO[1] + 54].sum() > 1: m[MO[1] + action[1]] = 0
    elif t == 1:
        if m[MO[2]:MO[2] + 73].sum() > 1: m[MO[2] + action[2]] = 0
    elif t == 2:
        if m[MO[1] + 54:MO[1] + 108].sum() > 1: m[MO[1] + 54 + action[1]] = 0
    elif t == 4:
        if m[MO[4]:MO[4] + 5].sum() > 1: m[MO[4] + action[4]] = 0
    elif t == 8:
        if m[MO[3]:MO[3] + 19].sum() > 0: m[MO[3] + action[3]] = 0
    elif t == 11:
        if m[MO[6] + 3:MO[6] + 6].sum() > 0: m[MO[6] + 3 + action[6]] = 0
    elif t == 12:
        if m[MO[11]:MO[11] + 5].sum() > 1: m[MO[11] + action[17]] = 0


@torch.no_grad()
def propose_actions(policy, f, lists, lens, masks, max_actions=10, initial_settlement_phase=None,
                    consider_all_initial_settlements=False, rngs=None, deterministic=False, generator=None, autocast_dtype=None,
                    hidden=None, return_hidden=False, dont_propose_devcards=False, dont_propose_trades=False):
    """default_sample_actions (sample_actions_fn.py:55-328) for R roots.  dont_propose_devcards: no BuyDevelopmentCard proposal,
    and where PlayDevelopmentCard is legal the previous proposal is listed a second time instead (:130,144-159: the reference's
    append sits outside its `if`); dont_propose_trades: no ProposeTrade proposal (:178).  f/lists/lens/masks: the roots' observations and masks (device tensors); rngs: one `random.Random` per root for
    the procedure's random.choice calls.  hidden (LSTM policies): (h, c) [R, L] each, the deciding seat's state; every proposal
    is sampled from it, and the state after the decision - the same for all proposals of a root, the LSTM step precedes the
    action heads - is returned with return_hidden (`player_next_hidden_states`, sample_actions_fn.py).
    -> (actions int64 numpy [R, A, 18], counts [R]) in proposal order [, (h, c) [R, L]]."""
    R, dev = f.shape[0], f.device
    m = masks.detach().cpu().numpy().astype(np.float32).copy()            # working copies, updated as targets are used up
    type_masks = m[:, MO[0]:MO[0] + 13].copy()
    rngs = rngs or [_py_random.Random(i) for i in range(R)]
    init_phase = np.zeros(R, dtype=bool) if initial_settlement_phase is None else np.asarray(initial_settlement_phase, dtype=bool)
    effective = np.zeros(R)
    trades = np.zeros(R, dtype=np.int64)

    rec = bool(getattr(policy, "include_lstm", False))
    if rec:
        Lh = int(policy.lstm_size)
        h_in = (torch.zeros(R, Lh, device=dev), torch.zeros(R, Lh, device=dev)) if hidden is None else (hidden[0].to(dev).float(), hidden[1].to(dev).float())
        h_next = (h_in[0].clone(), h_in[1].clone())

    def act(rows, types):
        idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
        forced = torch.as_tensor(types, device=dev, dtype=torch.long)
        mk = torch.from_numpy(m[rows]).to(dev)
        args = (f[idx], lists[idx], lens[idx].long(), mk)
        kw = {"hidden": (h_in[0][idx], h_in[1][idx]), "nonterminal": torch.ones(idx.numel(), device=dev)} if rec else {}
        res = acting.act(policy, args, autocast_dtype, deterministic=deterministic, generator=generator, condition_on_action_type=forced, **kw)
        if rec:
            h_next[0][idx], h_next[1][idx] = res[3][0].float(), res[3][1].float()
        return res[1].cpu().numpy()

    # Bookkeeping as arrays over the roots (round 1 walked Python dicts / lists per root: 1.5 s at 4 096 roots):
    #   avail [R, 13]   refinement draws left per type (sample_actions_fn.py `available_actions`; only refinable types > 0)
    #   props [R, cap, 18], n_prop [R]   the proposals in order;   ex [R, cap, 2], n_ex [R]   exchange pairs proposed so far
    REFINABLE = (0, 1, 2, 4, 5, 6, 8, 11, 12)
    cap = max(int(max_actions), 13) + (54 if consider_all_initial_settlements else 0) + 1
    avail = np.zeros((R, 13))
    props = np.zeros((R, cap, spec.ACTION_WORDS), dtype=np.int64); n_prop = np.zeros(R, dtype=np.int64)
    ex = np.zeros((R, cap, 2), dtype=np.int64); n_ex = np.zeros(R, dtype=np.int64)

    def counts_for(t, rows):
        """`count - 1` further targets of type t (sample_actions_fn.py:117-196), for all `rows` at once"""
        mr = m[rows]
        if t == 0: return mr[:, MO[1]:MO[1] + 54].sum(1) - 1
        if t == 1: return mr[:, MO[2]:MO[2] + 73].sum(1) - 1
        if t == 2: return mr[:, MO[1] + 54:MO[1] + 108].sum(1) - 1
        if t == 4: return mr[:, MO[4]:MO[4] + 5].sum(1) - 1
        if t == 5: return mr[:, MO[10]:MO[10] + 5].sum(1) * mr[:, MO[9]:MO[9] + 5].sum(1) - 1
        if t == 6: return np.full(len(rows), MAX_PROP_TRADE_ACTIONS - 1.0)
        if t == 8: return mr[:, MO[3]:MO[3] + 19].sum(1) - 1
        if t == 11: return mr[:, MO[6] + 3:MO[6] + 6].sum(1) - 1
        return mr[:, MO[11]:MO[11] + 5].sum(1) - 1                        # 12

    # _update_action_masks (sample_actions_fn.py:31-53) for many roots at once: (first mask column, width, action word, minimum sum)
    TARGET = {0: (MO[1], 54, 1, 1), 1: (MO[2], 73, 2, 1), 2: (MO[1] + 54, 54, 1, 1), 4: (MO[4], 5, 4, 1), 8: (MO[3], 19, 3, 0),
              11: (MO[6] + 3, 3, 6, 0), 12: (MO[11], 5, 17, 1)}

    def use_up(t, rows, acts):
        if t not in TARGET or len(rows) == 0:
            return
        lo, w, word, least = TARGET[t]
        rows = np.asarray(rows)
        ok = m[rows, lo:lo + w].sum(1) > least
        m[rows[ok], lo + acts[ok, word]] = 0

    def append(rows, acts):
        rows = np.asarray(rows)
        props[rows, n_prop[rows]] = acts
        n_prop[rows] += 1

    name_of = {v: k for k, v in TYPE_TO_IND.items()}
    for t in range(13):                                                   # first pass: one proposal per available type
        rows = np.flatnonzero(type_masks[:, t] == 1)
        if rows.size == 0:
            continue
        if (dont_propose_devcards and t == 3) or (dont_propose_trades and t == 6):      # :130, :178 - no proposal, nothing counted
            continue
        if dont_propose_devcards and t == 4:
            # :144-159: only the sampling is inside the `if`; the append below it runs again on the PREVIOUS proposal (a settlement,
            # road or city: its second mask update changes nothing).  A root with no earlier proposal raises UnboundLocalError in the
            # reference; here it gets no entry.
            rows = rows[n_prop[rows] > 0]
            if rows.size:
                append(rows, props[rows, n_prop[rows] - 1])
            continue
        if t in REFINABLE:
            c = counts_for(t, rows).astype(np.float64)
            avail[rows, t] = c
            effective[rows] += c
        elif t == 7:
            effective[rows] += m[rows, MO[5]:MO[5] + 2].sum(1) - 1         # respond: counted but not refinable (:198)
        a = act(rows, np.full(rows.size, t))
        assert (a[:, 0] == t).all()
        append(rows, a)
        if t == 5:
            ex[rows, n_ex[rows]] = a[:, 15:17]; n_ex[rows] += 1
        if t == 6:
            trades[rows] += 1
        use_up(t, rows, a)
    # refinement draws (:286-328)
    if consider_all_initial_settlements:
        n_more = np.where(init_phase, avail[:, 0].astype(np.int64), np.minimum(max_actions - n_prop, effective).astype(np.int64))
    else:
        n_more = np.minimum(max_actions - n_prop, effective).astype(np.int64)
    alive = n_more > 0
    prio = [[TYPE_TO_IND[x] for x in pr] for pr in PRIORITIES]
    for i in range(int(n_more.max()) if R else 0):
        rows, types = [], []
        for r in np.flatnonzero(alive & (i < n_more)):
            ac_type = -1
            av_r = avail[r]
            for pr in prio:
                av = [x for x in pr if av_r[x] > 0]
                if trades[r] >= MAX_PROP_TRADE_ACTIONS and 6 in av:
                    av.remove(6)
                if av:
                    ac_type = TYPE_TO_IND[rngs[r].choice([name_of[x] for x in av])]
                    av_r[ac_type] -= 1
                    break
            if ac_type < 0:
                alive[r] = False                                          # "something gone wrong - just return what we have"
                continue
            rows.append(r); types.append(ac_type)
        if not rows:
            break
        rows, types = np.asarray(rows), np.asarray(types)
        a = act(rows, types)
        is_ex = types == 5
        for j in np.flatnonzero(is_ex):
            # the reference re-draws the pair `while prop_exchange not in exchanges_proposed` (:316-320): a NEW pair is
            # replaced by random legal picks until it coincides with one proposed before
            r, act_j = rows[j], a[j]
            seen = {(int(x), int(y)) for x, y in ex[r, :n_ex[r]]}
            pair = (int(act_j[15]), int(act_j[16]))
            give_ok = np.flatnonzero(m[r, MO[9]:MO[9] + 5]); recv_ok = np.flatnonzero(m[r, MO[10]:MO[10] + 5])
            while pair not in seen:
                act_j[15] = rngs[r].choice(list(give_ok)); act_j[16] = rngs[r].choice(list(recv_ok))
                pair = (int(act_j[15]), int(act_j[16]))
            ex[r, n_ex[r]] = pair; n_ex[r] += 1
        append(rows, a)
        trades[rows[types == 6]] += 1
        for t in TARGET:
            sel = types == t
            if sel.any():
                use_up(t, rows[sel], a[sel])
    A = int(n_prop.max()) if R else 0
    out = props[:, :A].copy()
    counts = n_prop.copy()
    if return_hidden:
        return out, counts, (h_next if rec else None)
    return out, counts


# ---------------------------------------------------------------------------------------------------- the planner
class ForwardSearch(object):
    """ForwardSearchPolicy.act (policy.py:72-149) for all games of `root_env` at once - or for a sub-list of them (`games`) -,
    each searched by its deciding player.  make_sim_env(n) -> an env of n games with dense rewards and no auto-reset
    (VecCatanEnv on the GPU).

    state_broadcast: how a round's simulations get their start states.  "fork": catan_state_fork copies the packed records from
    the root env into the simulation env on the device (env.fork_from); "blob": catan_state_export once per decision, one blob per
    simulation, an edit of the draw-counter word and catan_state_import per round.  Both start every simulation from the same
    state with the same substream (draw counter = the root's + (1 + round * K + k) << 22), so they give identical simulations;
    an env without `fork_from` (the CPU test envs) always takes the blob path.

    What is kept PER GAME ID of the root env, so that it follows a game from one decision to the next whichever games are searched
    beside it: the Python `Random` of the proposals (`rngs`), the UCB counters and the value moving average (`stats`).
    One difference from the reference cannot be removed: the reference plays its evaluation games one after the other with ONE
    planner object, so `value_moving_average` (policy.py:47) carries over from game to game.  Here every game has a window of
    its own that starts empty, which is what the reference's first game sees.
    Simulation rows are handed out in ascending order of the game ids (rows j*K .. j*K+K-1 belong to the j-th smallest id), so the
    order in which `games` lists them changes nothing.  The dice of a simulation come from the simulation env's stream of its row:
    a game searched beside a different set of games may sit in another row and then sees other dice (the proposals, the UCB
    bookkeeping and the moving average do not move).  This departs from "the result for a game does not depend on which other
    games are searched beside it" and from "rows j*K .. belong to games[j]": the env's Philox streams are keyed by the handle's seed
    and the row, so only a per-game stream id in the simulation env would remove it."""

    def __init__(self, policy, make_sim_env, n_roots, max_init_actions=10, max_depth=20, gamma=0.999, sims_per_root=64,
                 sims_per_round=16, consider_all_moves_for_opening_placement=False, seed=0, autocast_dtype=None, use_graphs=False,
                 state_broadcast=DEFAULT_STATE_BROADCAST, dont_propose_devcards=False, dont_propose_trades=False):
        assert sims_per_root % sims_per_round == 0
        assert state_broadcast in ("fork", "blob"), state_broadcast
        if autocast_dtype is not None and hasattr(policy, "inference_copy") and getattr(policy, "_inference_dtype", None) is None:
            policy = policy.inference_copy(autocast_dtype)      # weights in the autocast dtype: no per-call casts
        self.policy, self.R = policy, n_roots
        self.max_init_actions, self.max_depth, self.gamma = max_init_actions, max_depth, gamma
        self.S, self.K = sims_per_root, sims_per_round
        self.consider_all = consider_all_moves_for_opening_placement
        self.dont_propose_devcards, self.dont_propose_trades = bool(dont_propose_devcards), bool(dont_propose_trades)
        self.state_broadcast = state_broadcast
        self.sim_env = make_sim_env(n_roots * sims_per_round)
        self.stats = UCBStats(n_roots, 54 if consider_all_moves_for_opening_placement else max_init_actions)
        self.seed = seed
        self.rngs = [_py_random.Random(seed * 1000003 + i) for i in range(n_roots)]       # indexed by game id (grown on demand)
        self.gen = None
        self.autocast_dtype = autocast_dtype
        params = getattr(policy, "parameters", None)
        if torch.cuda.is_available() and params is not None and next(params()).is_cuda:
            from . import nn_kernels
            nn_kernels.use_tuned_gemms()
        self.graphed = GraphedAct(policy, buckets=(512, 4096, 16384, 32768, 49152, 65536), autocast_dtype=autocast_dtype) if use_graphs else None
        self.sims_run = 0
        self._rng_word = spec.STATE_OFFSETS["rng_draws"][0]

    def _per_game(self, n_games):
        """the per-game-id state covers game ids 0 .. n_games-1"""
        while len(self.rngs) < n_games:
            self.rngs.append(_py_random.Random(self.seed * 1000003 + len(self.rngs)))
        self.stats.grow(n_games)

    @torch.no_grad()
    def act(self, root_env, initial_settlement=None, deterministic=False, hidden=None, zero_opponent_hidden_states=False,
            max_thinking_time=None, games=None):
        """-> (actions int64 numpy [R,18], info dict).  Roots with a single proposal skip the search (policy.py:88-89).
        games (device int64 [r], r <= n_roots, distinct ids into root_env, which may then hold more than n_roots games): only these
        games are searched; every per-root argument (initial_settlement, hidden) and every returned array then has r rows, in the
        order of `games`.  Simulation rows beyond r*K idle.
        LSTM policies: hidden [2, R, 4, L] = the (h, c) of every seat of every root (`curr_hidden_states`, policy.py:72; zeros if
        omitted); proposals and simulations run from them as the reference's do (:73-86, worker.py:61-95), and
        info["next_hidden"] [2, R, L] is the searching seat's state after its decision (`player_next_hidden_states`).
        max_thinking_time (seconds; None = the fixed budget of `sims_per_root`): the reference's wall-clock budget
        (policy.py:91,112-138): root r thinks for max_thinking_time * n_proposed[r] / max_init_actions; rounds of K simulations
        per root are run until the longest of those budgets is spent, and a root stops taking results once its own is."""
        K = self.K
        dev = root_env.device
        if games is None:
            assert root_env.n == self.R
            R = self.R
            ids = np.arange(R)
            pos = None
            gsel = None
        else:
            g_host = torch.as_tensor(games).cpu().numpy().astype(np.int64).reshape(-1)
            R = int(g_host.size)
            assert 0 < R <= self.R and np.unique(g_host).size == R and g_host.min() >= 0 and g_host.max() < root_env.n
            order = np.argsort(g_host, kind="stable")
            ids = g_host[order]                                                     # ascending game ids: the order of the simulation rows
            pos = np.empty(R, dtype=np.int64); pos[order] = np.arange(R)            # row of games[j] in that order
            gsel = torch.from_numpy(ids).to(dev)
            order_t = torch.from_numpy(order).to(dev)
            if initial_settlement is not None:
                initial_settlement = np.asarray(torch.as_tensor(initial_settlement).cpu().numpy() if torch.is_tensor(initial_settlement)
                                                else initial_settlement, dtype=bool)[order]
            if hidden is not None:
                hidden = hidden.to(dev)[:, order_t]
        self._per_game(int(ids.max()) + 1)
        stats = self.stats if games is None else self.stats.take(ids)
        rngs = self.rngs if games is None else [self.rngs[g] for g in ids]
        n_sim = self.sim_env.n
        live_rows = R * K
        ctrl = root_env.deciding_player().long()
        f, lists, lens = root_env.get_obs()
        masks = root_env.get_action_masks()
        if gsel is not None:
            ctrl, f, lists, lens, masks = ctrl[gsel], f[gsel], lists[gsel], lens[gsel], masks[gsel]
        rec = bool(getattr(self.policy, "include_lstm", False))
        hid_sim = init_sim = next_hidden = None
        if rec:
            Lh = int(self.policy.lstm_size)
            hidden = torch.zeros((2, R, 4, Lh), device=dev) if hidden is None else hidden.to(dev).float()
            ar_r = torch.arange(R, device=dev)
            own = (hidden[0, ar_r, ctrl - 1], hidden[1, ar_r, ctrl - 1])
        props, counts, nh = propose_actions(self.policy, f, lists, lens, masks, self.max_init_actions, initial_settlement, self.consider_all,
                                            rngs, deterministic, self.gen, self.autocast_dtype, hidden=own if rec else None, return_hidden=True,
                                            dont_propose_devcards=self.dont_propose_devcards, dont_propose_trades=self.dont_propose_trades)
        pad = n_sim - live_rows                                                     # idle simulation rows
        if rec:
            next_hidden = torch.stack(nh)                                           # [2, R, L]
            if zero_opponent_hidden_states:                                         # policy.py:81-86
                keep = torch.zeros((R, 4), dtype=torch.bool, device=dev)
                keep[ar_r, ctrl - 1] = True
                hidden = hidden * keep[None, :, :, None]
            hid_sim = hidden.repeat_interleave(K, dim=1)
            init_sim = next_hidden.repeat_interleave(K, dim=1)
            if pad:
                hid_sim = torch.cat((hid_sim, hid_sim.new_zeros((2, pad, 4, Lh))), 1)
                init_sim = torch.cat((init_sim, init_sim.new_zeros((2, pad, Lh))), 1)
        stats.new_decision(counts)
        use_fork = self.state_broadcast == "fork" and hasattr(self.sim_env, "fork_from") and hasattr(root_env, "fork_from")
        ar_sim = torch.arange(live_rows, device=dev)
        if use_fork:
            src_rows = (ar_sim // K) if gsel is None else gsel.repeat_interleave(K)
        else:
            blobs = export_games(root_env, gsel)                                   # [R, 736] int32 (state broadcast)
            blobs = blobs.repeat_interleave(K, dim=0).clone()
            base_draws = blobs[:, self._rng_word].long() & 0xFFFFFFFF
        ctrl_sim = ctrl.repeat_interleave(K)
        idle = None
        if pad:
            ctrl_sim = torch.cat((ctrl_sim, ctrl_sim.new_zeros(pad)))               # 0: randomise_uncertainty leaves the row alone
            idle = torch.arange(n_sim, device=dev) >= live_rows
        props_t = torch.from_numpy(props).to(dev)
        import time as _time
        t_start = _time.perf_counter()
        think = None if max_thinking_time is None else max_thinking_time * (counts / float(self.max_init_actions))      # policy.py:91
        rnd = -1
        while True:
            rnd += 1
            if think is None:
                if rnd >= self.S // K:
                    break
                thinking = np.ones(R, dtype=bool)
            else:
                thinking = (_time.perf_counter() - t_start) < think                 # `while elapsed_time < thinking_time`
                if not thinking.any():
                    break
            sel_ids = np.zeros((R, K), dtype=np.int64)
            for k in range(K):                                                      # one simulation after the other (:118-125)
                a = stats.select(explore=True)
                stats.start(a, np.flatnonzero(thinking))
                sel_ids[:, k] = a
            # every simulation its own philox substream: offset the game stream's draw counter by a large stride
            stride = ((1 + rnd * K + (ar_sim % K)) * (1 << 22)) & 0xFFFFFFFF
            if use_fork:
                self.sim_env.fork_from(root_env, src_rows, None, stride)            # worker.py:44-45, on the device
            else:
                sub = (base_draws + stride) & 0xFFFFFFFF
                blobs[:, self._rng_word] = torch.where(sub >= 2 ** 31, sub - 2 ** 32, sub).to(torch.int32)
                import_rows(self.sim_env, blobs)                                   # worker.py:44-45
            self.sim_env.randomise_uncertainty(ctrl_sim)                            # :46
            init = props_t[torch.arange(R, device=dev).repeat_interleave(K), torch.from_numpy(sel_ids.reshape(-1)).to(dev)]
            if pad:
                init = torch.cat((init, init.new_zeros((pad, init.shape[1]))))
            vals = simulate(self.sim_env, self.policy, ctrl_sim, init, self.max_depth, self.gamma, deterministic, self.gen,
                            self.autocast_dtype, None if deterministic else self.graphed, hidden=hid_sim, init_hidden=init_sim,
                            idle=idle)[:live_rows].reshape(R, K)
            rows = np.flatnonzero(thinking)
            for k in range(K):
                stats.update(vals[rows, k], sel_ids[rows, k], rows)
            self.sims_run += int(rows.size) * K
        best = stats.select(explore=False)
        best = np.where(counts == 1, 0, best)
        chosen = props[np.arange(R), best]
        info = {"n_proposed": counts, "best": best, "finished_each": stats.finished_each.copy(),
                "mean_value": stats.exploit / np.maximum(stats.finished_each, 1), "next_hidden": next_hidden}
        if games is not None:
            self.stats.put(ids, stats)
            chosen = chosen[pos]
            info = {k: (None if v is None else (v[:, torch.from_numpy(pos).to(v.device)] if torch.is_tensor(v) else v[pos])) for k, v in info.items()}
        return chosen, info


def export_games(env, games):
    """the canonical blobs of the games `games` (device int64; None: all) of a device env or a CPU test env"""
    if games is None:
        return env.export_state()
    if getattr(env, "takes_game_lists", False):                                     # export_state(env_idx) / import_state(blobs, env_idx)
        return env.export_state(games)
    return env.export_state()[games]


def import_rows(env, blobs):
    """blobs [m, 736] into the first m games of `env` (m <= env.n); the other games keep their states"""
    if blobs.shape[0] == env.n:
        env.import_state(blobs)
    elif getattr(env, "takes_game_lists", False):
        env.import_state(blobs, torch.arange(blobs.shape[0], device=blobs.device))
    else:                                                                           # an env that only imports all of its games
        full = env.export_state().clone()
        full[:blobs.shape[0]] = blobs
        env.import_state(full)
