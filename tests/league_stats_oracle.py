"""Expected league tables (catan_league_stats_*, include/catan_hip_tuning.h "league results") in plain Python, without any of the
library's statistics code: from episode records - the columns GAME, DECISION, WINNER and VP of episode_stats_oracle.replay - and the
two maps, for the episodes that lie within each game's counter (lock-step: the number of steps; deferred: the game's policy counter)."""
import numpy as np

import episode_stats_oracle as eso

GAMES, SEATS, NET_WINS, CENTRAL_WINS, NET_VP, CENTRAL_VP = range(6)
T_SEEN, T_TALLIED, T_CENTRAL_WINS, T_CENTRAL_VP, T_SKIPPED_GAMES, T_SKIPPED_SEATS = range(6)


def tally_game(table, winner, vp, slots, nets, num_nets):
    """adds one finished game to `table` (list of num_nets + 1 lists of 6 ints): winner PlayerId (0: none), vp[4] by PlayerId-1,
    slots[4] the policy slot of PlayerId p+1, nets[3] the net of slots 1..3"""
    tot = table[num_nets]
    tot[T_SEEN] += 1
    slots = [int(x) for x in slots]
    if not 1 <= winner <= 4 or sorted(slots) != [0, 1, 2, 3]:
        tot[T_SKIPPED_GAMES] += 1
        return
    central = slots.index(0)
    tot[T_TALLIED] += 1
    tot[T_CENTRAL_WINS] += int(central == winner - 1)
    tot[T_CENTRAL_VP] += int(vp[central])
    met = set()
    for j in (1, 2, 3):
        k = int(nets[j - 1])
        if k == -1:
            continue
        if not 0 <= k < num_nets:
            tot[T_SKIPPED_SEATS] += 1
            continue
        seat = slots.index(j)
        row = table[k]
        if k not in met:
            row[GAMES] += 1
            met.add(k)
        row[SEATS] += 1
        row[NET_WINS] += int(seat == winner - 1)
        row[CENTRAL_WINS] += int(central == winner - 1)
        row[NET_VP] += int(vp[seat])
        row[CENTRAL_VP] += int(vp[central])


def table(ep, counts, slot_of_pid, net_of_slot, num_nets):
    """-> int64 [num_nets + 1][6]: the episodes of `ep` (rows of episode_stats_oracle.replay) with DECISION <= counts[game]
    (counts: one number for all games, or one per game)"""
    ep = np.asarray(ep, dtype=np.int64).reshape(-1, eso.COLS)
    n = len(slot_of_pid)
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (n,))
    t = [[0] * 6 for _ in range(num_nets + 1)]
    for r in ep:
        g = int(r[eso.GAME])
        if r[eso.DECISION] <= counts[g]:
            tally_game(t, int(r[eso.WINNER]), [int(x) for x in r[eso.VP:eso.VP + 4]], slot_of_pid[g], net_of_slot[g], num_nets)
    return np.array(t, dtype=np.int64)


def table_of_states(winner, vp, games, slot_of_pid, net_of_slot, num_nets):
    """-> the table of the listed games' current states (catan_league_stats_count): winner [n], vp [n][4]"""
    t = [[0] * 6 for _ in range(num_nets + 1)]
    for g in games:
        g = int(g)
        tally_game(t, int(winner[g]), [int(x) for x in vp[g]], slot_of_pid[g], net_of_slot[g], num_nets)
    return np.array(t, dtype=np.int64)


def maps(n, num_nets, seed, minus_one_every=7, bad_game=None):
    """The fixed maps of the tests: a random seat permutation per game and random nets, every `minus_one_every`-th seat -1, and
    (bad_game) one game whose slot row is no permutation.  -> (slot_of_pid int32 [n,4], net_of_slot int32 [n,3])"""
    rs = np.random.RandomState(seed)
    slot = np.stack([rs.permutation(4) for _ in range(n)]).astype(np.int32)
    net = rs.randint(0, num_nets, size=(n, 3)).astype(np.int32)
    flat = net.reshape(-1)
    flat[::minus_one_every] = -1
    if bad_game is not None:
        slot[bad_game] = [0, 1, 1, 3]
    return slot, net
