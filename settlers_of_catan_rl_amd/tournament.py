"""Round-robin tournaments on the device, and ratings from their tables (no counterpart in the reference).

M players - nets, the rule-based players, the uniform-random sampler, anything `acting.act` can call - meet in LINEUPS of four.  The
env seats every game by a rule without a draw (csrc/catan_hooks.hip: every lineup meets every seat permutation equally often), books
every finished game by who sat where in front of its re-deal, and seats the re-dealt game anew: `run_tournament` streams games on an
env with auto_reset and never waits for a batch's longest game.  `fit_ratings` turns the table into Plackett-Luce strengths on first
place, reported as Elo-like ratings with standard errors; `report` prints both."""
import itertools
import math

import numpy as np
import torch

from . import acting, spec

MAX_LINEUPS = spec.TOURNAMENT_MAX_LINEUPS
CHECK_EVERY = 32                 # passes between two looks of run_tournament at the table (its one host read) and at the step cap


# ---------------------------------------------------------------- lineups
def check_lineups(lineups, num_players=None):
    """-> int64 [L, 4]; ValueError for another shape, no row, more than 65 536 rows or an id outside [0, num_players)"""
    a = np.asarray(lineups, dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1:
        raise ValueError(f"lineups: shape [L, 4] with L >= 1 expected, got {tuple(a.shape)}")
    if a.shape[0] > MAX_LINEUPS:
        raise ValueError(f"{a.shape[0]} lineups: the table takes at most {MAX_LINEUPS}")
    if a.min() < 0 or (num_players is not None and a.max() >= num_players):
        raise ValueError(f"lineups: player ids must be in 0..{'' if num_players is None else num_players - 1}")
    return a


def all_lineups(num_players):
    """Every 4-subset of the players, in lexicographic order; with fewer than four players every multiset of size 4 -> int64 [L, 4]"""
    m = int(num_players)
    if m < 1:
        raise ValueError("all_lineups: at least one player")
    count = math.comb(m, 4) if m >= 4 else math.comb(m + 3, 4)
    if count > MAX_LINEUPS:
        raise ValueError(f"all_lineups({m}) is {count} lineups: the table takes at most {MAX_LINEUPS}")
    rows = itertools.combinations(range(m), 4) if m >= 4 else itertools.combinations_with_replacement(range(m), 4)
    return check_lineups(list(rows), m)


def versus_anchors(candidates, anchors):
    """Each candidate against fixed players: [c, a, a, a] for every candidate c and anchor a, and - with at least three anchors - c
    against the first three together -> int64 [L, 4], candidate-major"""
    candidates, anchors = [int(c) for c in candidates], [int(a) for a in anchors]
    if not candidates or not anchors:
        raise ValueError("versus_anchors: at least one candidate and one anchor")
    per = len(anchors) + (1 if len(anchors) >= 3 else 0)
    if len(candidates) * per > MAX_LINEUPS:
        raise ValueError(f"versus_anchors: {len(candidates) * per} lineups, the table takes at most {MAX_LINEUPS}")
    rows = []
    for c in candidates:
        rows += [[c, a, a, a] for a in anchors]
        if len(anchors) >= 3:
            rows.append([c] + anchors[:3])
    return check_lineups(rows)


# ---------------------------------------------------------------- the seat rule, restated for the a-priori counts
SEAT_PERMUTATIONS = tuple(itertools.permutations(range(4)))          # lexicographic: entry p = the lineup position PlayerId p+1 plays


def seating(s, num_lineups):
    """-> (lineup, permutation) of the episode with index s (the library's rule)"""
    s &= (1 << 64) - 1
    return s % num_lineups, SEAT_PERMUTATIONS[(s // num_lineups) % 24]


def episode_index(game_id, k, episodes_per_game):
    """s of the k-th episode (from 0) of the game with global id game_id"""
    return (game_id * episodes_per_game + k if episodes_per_game else game_id + (k << 32)) & ((1 << 64) - 1)


def expected_games(n, episodes_per_game, num_lineups, env_id0=0):
    """-> int64 [L]: the episodes each lineup plays when n games (ids from env_id0) play episodes_per_game > 0 episodes each"""
    out = np.zeros(num_lineups, dtype=np.int64)
    for g in range(n):
        for k in range(episodes_per_game):
            out[seating(episode_index(env_id0 + g, k, episodes_per_game), num_lineups)[0]] += 1
    return out


# ---------------------------------------------------------------- the streaming loop
@torch.no_grad()
def run_tournament(env, players, lineups, episodes_per_game, max_steps=2500, deterministic=False, generator=None, autocast_dtype=None):
    """Plays `episodes_per_game` episodes in each of the env's game slots (an env with auto_reset, stepped lock-step), the seats of every
    episode taken by `players` as the env's seat rule says, and returns when every game has retired.
    players: M policies; one `acting.act` call per player and pass over the rows it decides.  A player with `wants_games`
    (scripted.GamesPolicy) gets the row -> game map and is bound to the env; an LSTM net keeps one (h, c) per game and seat, zeroed when
    the game's done flag comes back.  lineups: int [L, 4] (all_lineups, versus_anchors).  max_steps: a game that has taken more env
    steps is reset (env.reset(mask)) at the loop's next check, booked as a draw and seated anew - a draw uses up an episode like any
    game.  Retired games are stepped with the no-op.
    Every CHECK_EVERY passes the loop reads the table - its only host read beyond the row counts - and ends once the totals row says all
    n games have retired.
    -> {"table": int64 [L + 1, 16] (spec.TOURNAMENT_FIELDS / TOURNAMENT_TOTALS), "lineups", "players": summarise(...), "passes"}"""
    lineups = check_lineups(lineups, len(players))
    if int(episodes_per_game) < 1:
        raise ValueError("run_tournament: episodes_per_game must be at least 1 (an unlimited tournament never ends)")
    n, dev = env.n, env.device
    if autocast_dtype is not None:
        players = [p.inference_copy(autocast_dtype) if (hasattr(p, "inference_copy") and getattr(p, "_inference_dtype", None) is None) else p
                   for p in players]
    for p in players:
        if getattr(p, "wants_games", False) and hasattr(p, "rebind"):
            p.rebind(env)
    env.enable_tournament(lineups, len(players), int(episodes_per_game))
    env.reset()
    lineup_of, pos_of_pid = env.tournament_seating()
    lt = torch.as_tensor(lineups, device=dev)
    ar = torch.arange(n, device=dev)
    steps = torch.zeros(n, dtype=torch.long, device=dev)
    sizes = [int(p.lstm_size) for p in players if getattr(p, "include_lstm", False)]
    hid = torch.zeros((2, n, 4, max(sizes)), dtype=torch.float32, device=dev) if sizes else None
    idle = torch.full((n,), -1, dtype=torch.int32, device=dev)
    retired_col = spec.TOURNAMENT_TOTALS.index("retired")
    passes = 0
    while True:
        deciding = env.deciding_player().long()
        lo = lineup_of.long()
        seated = lo >= 0
        pos = pos_of_pid.long()[ar, deciding - 1]
        pid = torch.where(seated, lt[lo.clamp(min=0), pos.clamp(min=0)], torch.full_like(lo, -1))
        f, lists, lens = env.get_obs()
        masks = env.get_action_masks()
        actions = torch.zeros((n, spec.ACTION_WORDS), dtype=torch.int64, device=dev)
        for k, net in enumerate(players):
            idx = (pid == k).nonzero(as_tuple=True)[0]
            if idx.numel() == 0:
                continue
            kw = {"deterministic": deterministic, "generator": generator}
            if getattr(net, "wants_games", False):
                kw["games"] = idx
            rec = getattr(net, "include_lstm", False)
            if rec:
                L, seat = int(net.lstm_size), deciding[idx] - 1
                kw.update(hidden=(hid[0, idx, seat, :L], hid[1, idx, seat, :L]), nonterminal=torch.ones(idx.numel(), device=dev))
            res = acting.act(net, (f[idx], lists[idx], lens[idx].long(), masks[idx]), autocast_dtype, **kw)
            actions[idx] = res[1].long()
            if rec:
                hid[0, idx, seat, :L], hid[1, idx, seat, :L] = res[3][0].float(), res[3][1].float()
        a_env = actions.to(torch.int32)
        a_env[:, 0] = torch.where(seated, a_env[:, 0], idle)
        _, done = env.step(a_env)
        done = done.bool() & seated
        steps = torch.where(done, torch.zeros_like(steps), steps + seated.long())
        if hid is not None:
            hid *= (~done)[None, :, None, None]
        passes += 1
        if passes % CHECK_EVERY:
            continue
        if passes > max_steps:                           # (no game can be past the cap earlier)
            capped = steps > max_steps                   # (a retired game's count stands still at 0: its last game ended)
            env.reset(capped)
            steps = torch.where(capped, torch.zeros_like(steps), steps)
            if hid is not None:
                hid *= (~capped)[None, :, None, None]
        if int(env.tournament_table()[-1, retired_col]) == n:
            break
    table = env.tournament_table().clone()
    env.disable_tournament()
    return {"table": table, "lineups": lineups, "players": summarise(table, lineups, len(players)), "passes": passes}


def summarise(table, lineups, num_players):
    """-> one dict per player over the lineups it sits in: games (decided games, once per game), draws, wins, share (wins / games),
    fair_share (what equal players would win given its lineups: the mean of its multiplicity / 4 over its games), mean_vp (per seat),
    wins_by_turn (those games' winners by their place in the turn order, whoever won) and mean_turns.  NaN where it played no game."""
    t = np.asarray(table, dtype=np.int64)
    lineups = check_lineups(lineups, num_players)
    rows = t[:len(lineups)]
    decided = rows[:, spec.TOURNAMENT_GAMES] - rows[:, spec.TOURNAMENT_DRAWS]
    out = []
    for i in range(num_players):
        mine = lineups == i                                              # [L, 4]
        mult = mine.sum(1)
        games = int(decided[mult > 0].sum())
        wins = int((rows[:, spec.TOURNAMENT_WINS:spec.TOURNAMENT_WINS + 4] * mine).sum())
        vp = int((rows[:, spec.TOURNAMENT_VP:spec.TOURNAMENT_VP + 4] * mine).sum())
        seats = int((decided * mult).sum())
        div = lambda a, b: float(a) / b if b else float("nan")
        out.append({"player": i, "games": games, "draws": int(rows[mult > 0, spec.TOURNAMENT_DRAWS].sum()), "wins": wins,
                    "share": div(wins, games), "fair_share": div(seats / 4.0, games), "mean_vp": div(vp, seats),
                    "wins_by_turn": [int(x) for x in rows[mult > 0, spec.TOURNAMENT_WINS_BY_TURN:spec.TOURNAMENT_WINS_BY_TURN + 4].sum(0)],
                    "mean_turns": div(int(rows[mult > 0, spec.TOURNAMENT_TURNS].sum()), games)})
    return out


# ---------------------------------------------------------------- ratings
RATING_SCALE = 400.0 / math.log(10.0)            # rating points per unit of log-strength
MM_TOLERANCE, MM_MAX_ITERATIONS = 1e-12, 10000


def fit_ratings(table, lineups, num_players, anchor=0, prior_games=1.0):
    """Plackett-Luce on first place over the decided games: P(position j wins | lineup l) = s_lj / sum_m s_lm, the sum over the lineup's
    four seats (a player that holds several counts once per seat).  Maximum likelihood by Hunter's MM iteration (Ann. Statist. 32, 2004)
    in float64 - s_i <- W_i / sum_l N_l c_li / S_l with W_i the player's wins, N_l the lineup's decided games, c_li its seats in it and
    S_l the lineup's strength sum at the current iterate -, normalised to s_anchor = 1 after every sweep, until max |delta log s| <
    1e-12 or 10 000 sweeps.
    prior_games: that many virtual two-player games between every other player and the anchor, half won by each - a weak pull towards
    the anchor that keeps a winless (or unbeaten) player finite.  A default, not a tuned value; 0 gives the plain maximum likelihood.
    -> {"log_strength" [M] (anchor 0), "rating" = 400 log10(s_i / s_anchor), "stderr" (rating points; from the inverse of the observed
    information in the log-strengths with the anchor fixed, the prior's games included; the anchor's is 0; NaN where the information is
    singular), "converged", "iterations", "wins" [M], "games" (decided, total)}"""
    lineups = check_lineups(lineups, num_players)
    m, anchor, prior = int(num_players), int(anchor), float(prior_games)
    if not 0 <= anchor < m:
        raise ValueError(f"fit_ratings: anchor {anchor} outside 0..{m - 1}")
    t = np.asarray(table, dtype=np.float64)
    wins_pos = t[:len(lineups), spec.TOURNAMENT_WINS:spec.TOURNAMENT_WINS + 4]              # [L, 4]
    n_l = wins_pos.sum(1)                                                                    # decided games per lineup
    c = np.zeros((len(lineups), m))                                                          # seats of player i in lineup l
    w = np.zeros(m)
    for j in range(4):
        np.add.at(c, (np.arange(len(lineups)), lineups[:, j]), 1.0)
        np.add.at(w, lineups[:, j], wins_pos[:, j])
    others = np.arange(m) != anchor
    w_all = w + prior / 2.0 * others
    w_all[anchor] += prior / 2.0 * others.sum()
    s = np.ones(m)
    converged, it = False, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(1, MM_MAX_ITERATIONS + 1):
            denom = (n_l / (c @ s)) @ c                                                      # sum_l N_l c_li / S_l
            pair = prior / (s + s[anchor]) * others                                          # the virtual games of i against the anchor
            denom = denom + pair
            denom[anchor] += pair.sum()
            new = np.where(w_all > 0, w_all / denom, 0.0)
            new = new / new[anchor]
            delta = np.abs(np.log(new[(new > 0) & (s > 0)]) - np.log(s[(new > 0) & (s > 0)]))
            moved = bool(((new > 0) != (s > 0)).any())
            s = new
            if not moved and (delta.size == 0 or delta.max() < MM_TOLERANCE):
                converged = True
                break
        theta = np.log(s)
        # observed information in theta = log s: sum_l N_l (diag(q_l) - q_l q_l^T), q_li = c_li s_i / S_l, and the same for the prior's pairs
        q = c * s / (c @ s)[:, None]
        info = np.diag(n_l @ q) - (q * n_l[:, None]).T @ q
        for i in np.flatnonzero(others):
            if prior > 0 and s[i] > 0:
                p = s[i] / (s[i] + s[anchor])
                h = prior * p * (1.0 - p)
                info[i, i] += h; info[anchor, anchor] += h; info[i, anchor] -= h; info[anchor, i] -= h
        stderr = np.full(m, np.nan)
        stderr[anchor] = 0.0
        keep = np.flatnonzero(others)
        try:
            if keep.size and np.isfinite(info).all():
                cov = np.linalg.inv(info[np.ix_(keep, keep)])
                d = np.diag(cov)
                stderr[keep] = np.where(d > 0, np.sqrt(np.abs(d)), np.nan) * RATING_SCALE
        except np.linalg.LinAlgError:
            pass
    return {"log_strength": theta, "rating": theta * RATING_SCALE, "stderr": stderr, "converged": converged, "iterations": it,
            "wins": w, "games": float(n_l.sum()), "anchor": anchor, "prior_games": prior}


def report(result, names=None, ratings=None):
    """-> the text table of a run_tournament result (and of fit_ratings' output where given): one line per player"""
    players = result["players"] if isinstance(result, dict) and "players" in result else result
    names = [str(p["player"]) for p in players] if names is None else [str(x) for x in names]
    width = max(8, max(len(x) for x in names))
    head = f"{'player':<{width}} {'games':>7} {'draws':>6} {'wins':>7} {'share':>7} {'fair':>7} {'mean vp':>8} {'turns':>7}"
    if ratings is not None:
        head += f" {'rating':>8} {'+/-':>7}"
    lines = [head]
    for p, name in zip(players, names):
        line = (f"{name:<{width}} {p['games']:>7d} {p['draws']:>6d} {p['wins']:>7d} {p['share']:>7.3f} {p['fair_share']:>7.3f} "
                f"{p['mean_vp']:>8.2f} {p['mean_turns']:>7.1f}")
        if ratings is not None:
            line += f" {ratings['rating'][p['player']]:>8.1f} {ratings['stderr'][p['player']]:>7.1f}"
        lines.append(line)
    if ratings is not None:
        lines.append(f"ratings: 400 log10(s / s_anchor), anchor {names[ratings['anchor']]} = 0, {ratings['games']:.0f} decided games, "
                     f"prior_games {ratings['prior_games']:g}, "
                     + (f"converged in {ratings['iterations']} sweeps" if ratings["converged"] else f"NOT converged after {ratings['iterations']} sweeps"))
    return "\n".join(lines)
