"""The rule-based "trader" player restated in numpy: test infrastructure for the device kernel k_sample_trader.

Works from an exported state blob and the float masks [325], as tests/scripted_reference.py does for the builder, whose rows it takes
from there; shares no code with the kernel.  `decide(blob, masks)` -> (action int32 [18], row): the builder's row number 1..13, or one
of the three new rows "2T", "11P", "11E".  `Tally` adds up the eight counters of catan_scripted_trade_counts."""
import numpy as np

import scripted_reference as sr
from settlers_of_catan_rl_amd import spec

ACCEPT = 0
VP_CAP = 8
MAX_ROADS = 15
GOALS = ("city", "settlement", "road", "devcard")
#        Brick Wood Ore Sheep Wheat
COSTS = ((0, 0, 3, 0, 2), (1, 1, 0, 1, 1), (1, 1, 0, 0, 0), (0, 0, 1, 1, 1))
COUNT_KEYS = ("decisions", "proposals", "responses", "accepts", "rejects_illegal", "rejects_other", "goal_exchanges", "fallbacks")


def _f(blob, name):
    return spec.state_field(blob, name)


def deficit(cost, h):
    return sum(max(0, c - x) for c, x in zip(cost, h))


def goal_of(blob, me, h):
    """-> index into GOALS / COSTS of the available goal with the smallest deficit (ties in table order), or None"""
    bld, own = _f(blob, "corner_bld"), _f(blob, "corner_owner")
    site = sr.has_open_site(blob, me)
    roads = int((_f(blob, "edge_owner") == me + 1).sum())
    avail = (bool(((bld == 1) & (own == me + 1)).any()) and int(_f(blob, "cities_left")[me]) > 0,
             site and int(_f(blob, "settlements_left")[me]) > 0,
             (not site) and roads < MAX_ROADS,
             int(_f(blob, "pile_len")[0]) > 0)
    best = None
    for g in range(4):
        if avail[g] and (best is None or deficit(COSTS[g], h) < deficit(COSTS[best], h)):
            best = g
    return best


def rate(blob, me, r):
    hb = _f(blob, f"p{me + 1}_harbours")
    return 2 if hb[r + 1] else (3 if hb[0] else 4)


def _pick(cands, key):
    """the candidate with the largest key > 0; ties to the lowest; None if there is none"""
    best = None
    for r in cands:
        if key[r] > 0 and (best is None or key[r] > key[best]):
            best = r
    return best


RESPOND_CONDITIONS = ("accept is legal", "n_recv <= n_give", "proposer below 8 points", "a goal", "the deficit falls")


def respond_conditions(blob, masks):
    """row 2T's five conditions for the open offer, in the order of RESPOND_CONDITIONS -> five bools (accept: all of them)"""
    me = sr.deciding_pid0(blob)
    h = [int(x) for x in _f(blob, f"p{me + 1}_res")]
    g = goal_of(blob, me, h)
    ng, nr = int(_f(blob, "trade_n_give")[0]), int(_f(blob, "trade_n_recv")[0])
    h2 = list(h)
    for v in _f(blob, "trade_give")[:ng]:
        h2[int(v) - 1] += 1
    for v in _f(blob, "trade_recv")[:nr]:
        h2[int(v) - 1] -= 1
    proposer = int(_f(blob, "trade_proposer")[0]) - 1
    return (bool(sr._head(masks, 5)[ACCEPT]), nr <= ng, int(_f(blob, "curr_vps")[proposer]) < VP_CAP, g is not None,
            g is not None and deficit(COSTS[g], h2) < deficit(COSTS[g], h))


def decide(blob, masks):
    blob = np.asarray(blob)
    a, row = sr.decide(blob, masks)
    if row != 2 and row < 11:
        return a, row
    types = sr._head(masks, 0)
    me = sr.deciding_pid0(blob)
    h = [int(x) for x in _f(blob, f"p{me + 1}_res")]
    g = goal_of(blob, me, h)
    if row == 2:
        a[5] = ACCEPT if all(respond_conditions(blob, masks)) else sr.REJECT
        return a, "2T"
    if g is not None and deficit(COSTS[g], h) >= 1:
        need = [max(0, c - x) for c, x in zip(COSTS[g], h)]
        spare = [max(0, x - c) for c, x in zip(COSTS[g], h)]
        if types[sr.PROPOSE] and any(spare):
            want, give = _pick(range(5), need), _pick(range(5), spare)
            order = [int(x) for x in _f(blob, "player_order")]
            seat = order.index(me + 1)
            vps = _f(blob, "curr_vps")
            cands = []
            for label in range(3):
                p = order[(seat + 1 + label) % 4]
                if int(_f(blob, f"p{p}_res")[want]) >= 1 and int(vps[p - 1]) < VP_CAP:
                    cands.append((int(vps[p - 1]), label))
            cands.sort()
            k = int(_f(blob, "trades_this_turn")[0])
            if k < len(cands):
                a = np.zeros(18, dtype=np.int32)
                a[0], a[6], a[7], a[11] = sr.PROPOSE, cands[k][1], give + 1, want + 1
                return a, "11P"
        if types[sr.EXCHANGE]:
            h9, h10 = sr._head(masks, 9)[0], sr._head(masks, 10)
            give = _pick([r for r in range(5) if h9[r] and spare[r] >= rate(blob, me, r)], spare)
            want = _pick([r for r in range(5) if h10[r]], need)
            if give is not None and want is not None:
                a = np.zeros(18, dtype=np.int32)
                a[0], a[15], a[16] = sr.EXCHANGE, give, want
                return a, "11E"
    return a, row


class Tally(object):
    """the eight counters of catan_scripted_trade_counts, from the decisions the twin takes"""

    def __init__(self):
        self.c = dict.fromkeys(COUNT_KEYS, 0)

    def add(self, a, row, masks):
        c = self.c
        c["decisions"] += 1
        if row == "11P":
            c["proposals"] += 1
        elif row == "11E":
            c["goal_exchanges"] += 1
        elif row == 13:
            c["fallbacks"] += 1
        elif row == "2T":
            c["responses"] += 1
            if a[5] == ACCEPT:
                c["accepts"] += 1
            elif not sr._head(masks, 5)[ACCEPT]:
                c["rejects_illegal"] += 1
            else:
                c["rejects_other"] += 1


def decide_all(blobs, masks, tally=None):
    """-> (actions int32 [n,18], rows list [n])"""
    out = [decide(b, m) for b, m in zip(np.asarray(blobs), np.asarray(masks))]
    if tally is not None:
        for (a, row), m in zip(out, np.asarray(masks)):
            tally.add(a, row, m)
    return np.stack([a for a, _ in out]), [r for _, r in out]
