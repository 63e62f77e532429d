"""The rule-based "builder" player restated in numpy: test infrastructure for the device kernel k_sample_scripted.

Works from an exported state blob (spec.STATE_OFFSETS), the float masks [325] and tests/golden/topology.npz; shares no code with the
kernel (no bitboards, no packed masks: plain per-corner / per-edge arrays).  `decide(blob, masks)` -> (action int32 [18], row of the
table 1..13)."""
import os

import numpy as np

from settlers_of_catan_rl_amd import spec

_T = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology.npz"))
CORNER_TILE, CORNER_NBR, CORNER_EDGE = _T["corner_tile"], _T["corner_nbr_corner"], _T["corner_nbr_edge"]
EDGE_CORNER, TILE_CORNER = _T["edge_corner"], _T["tile_corner"]

# ActionTypes / DevelopmentCard of the reference (game/enums.py)
SETTLE, ROAD, CITY, BUYDEV, PLAYDEV, EXCHANGE, PROPOSE, RESPOND, ROBBER, ROLL, ENDTURN, STEAL, DISCARD = range(13)
KNIGHT, VICTORY_POINT, YEAR_OF_PLENTY, ROAD_BUILDING, MONOPOLY = range(5)
REJECT = 1                       # env/wrapper.py:159-160: action[5] == 1 is "reject"
DUMMY_EDGE = 72


def _f(blob, name):
    return spec.state_field(blob, name)


def _head(masks, h):
    o = spec.MASK_OFFSETS[h]
    return np.asarray(masks[o:o + spec.MASK_SIZES[h]]).reshape(spec.MASK_SHAPES[h]) > 0


def pips(blob):
    res, val = _f(blob, "tile_res"), _f(blob, "tile_val")
    return np.array([0 if res[t] == 0 else max(0, 6 - abs(7 - int(val[t]))) for t in range(19)])


def corner_values(blob):
    p = pips(blob)
    return np.array([sum(int(p[t]) for t in CORNER_TILE[c] if t >= 0) for c in range(54)])


def corner_kinds(blob):
    res = _f(blob, "tile_res")
    return np.array([len({int(res[t]) for t in CORNER_TILE[c] if t >= 0 and res[t] != 0}) for c in range(54)])


def deciding_pid0(blob):
    if int(_f(blob, "n_to_discard")[0]) > 0:
        return int(_f(blob, "to_discard")[0]) - 1
    if int(_f(blob, "must_respond")[0]):
        return int(_f(blob, "trade_target")[0]) - 1
    return int(_f(blob, "players_go")[0]) - 1


def _argbest(cands, key):
    """the candidate with the largest key (a tuple); ties to the earliest candidate (they come in ascending index order)"""
    best, bk = None, None
    for c in cands:
        k = key(c)
        if best is None or k > bk:
            best, bk = c, k
    return best


def _free_corners(blob):
    """empty corners with no building on a neighbouring corner"""
    bld = _f(blob, "corner_bld")
    return [c for c in range(54) if bld[c] == 0 and all(bld[n] == 0 for n in CORNER_NBR[c] if n >= 0)]


def has_open_site(blob, me):
    eo = _f(blob, "edge_owner")
    return any(any(e >= 0 and eo[e] == me + 1 for e in CORNER_EDGE[c]) for c in _free_corners(blob))


def _lowest(bits):
    idx = np.flatnonzero(bits)
    return int(idx[0]) if idx.size else 0


def decide(blob, masks):
    blob = np.asarray(blob)
    a = np.zeros(18, dtype=np.int32)
    types = _head(masks, 0)
    me = deciding_pid0(blob)
    hand = [int(x) for x in _f(blob, f"p{me + 1}_res")]

    def legal_res(bits):
        return [r for r in range(5) if bits[r]]

    if types[DISCARD]:
        a[0] = DISCARD
        a[17] = _argbest(legal_res(_head(masks, 11)), lambda r: (hand[r],)) or 0
        return a, 1
    if types[RESPOND]:
        a[0], a[5] = RESPOND, REJECT
        return a, 2
    if types[STEAL]:
        order = [int(x) for x in _f(blob, "player_order")]
        seat = order.index(me + 1)
        vps = _f(blob, "curr_vps")

        def key(label):
            p = order[(seat + 1 + label) % 4]
            return (int(_f(blob, f"p{p}_res").sum()), int(vps[p - 1]))
        a[0] = STEAL
        a[6] = _argbest([l for l in range(3) if _head(masks, 6)[1, l]], key) or 0
        return a, 3
    if types[ROBBER]:
        p, bld, own = pips(blob), _f(blob, "corner_bld"), _f(blob, "corner_owner")

        def score(t):
            mine = sum(int(bld[c]) for c in TILE_CORNER[t] if own[c] == me + 1)
            others = sum(int(bld[c]) for c in TILE_CORNER[t] if own[c] not in (0, me + 1))
            return (-1000 if mine else int(p[t]) * others,)
        a[0] = ROBBER
        a[3] = _argbest([t for t in range(19) if _head(masks, 3)[t]], score) or 0
        return a, 4
    if types[ROLL]:
        a[0] = ROLL
        return a, 5
    if types[CITY]:
        cv = corner_values(blob)
        a[0] = CITY
        a[1] = _argbest([c for c in range(54) if _head(masks, 1)[1, c]], lambda c: (int(cv[c]),)) or 0
        return a, 6
    if types[SETTLE]:
        cv, ck = corner_values(blob), corner_kinds(blob)
        a[0] = SETTLE
        a[1] = _argbest([c for c in range(54) if _head(masks, 1)[0, c]], lambda c: (int(cv[c]), int(ck[c]))) or 0
        return a, 7
    if types[PLAYDEV]:
        cards = _head(masks, 4)
        playable = [cd for cd in (KNIGHT, ROAD_BUILDING, YEAR_OF_PLENTY, MONOPOLY) if cards[cd]]
        if playable:
            cd = playable[0]
            a[0], a[4] = PLAYDEV, cd
            if cd == YEAR_OF_PLENTY:
                h9, h10 = _head(masks, 9)[3], _head(masks, 10)
                first = legal_res(h9 & h10) or legal_res(h9)
                a[15] = _argbest(first, lambda r: (-hand[r],)) or 0
                held = list(hand)
                held[int(a[15])] += 1
                a[16] = _argbest(legal_res(h10), lambda r: (-held[r],)) or 0
            elif cd == MONOPOLY:
                theirs = [sum(int(_f(blob, f"p{p + 1}_res")[r]) for p in range(4) if p != me) for r in range(5)]
                a[15] = _argbest(legal_res(_head(masks, 9)[2]), lambda r: (theirs[r],)) or 0
            return a, 8
    if types[BUYDEV]:
        a[0] = BUYDEV
        return a, 9
    if types[ROAD]:
        only = not any(types[t] for t in range(13) if t not in (ROAD, ENDTURN))
        if only or not has_open_site(blob, me):
            cv, free = corner_values(blob), set(_free_corners(blob))
            edges = _head(masks, 2)
            real = [e for e in range(72) if edges[e]]
            a[0] = ROAD
            if real:
                a[2] = _argbest(real, lambda e: (max([int(cv[c]) for c in EDGE_CORNER[e] if c in free] + [-1]),))
            else:
                a[2] = DUMMY_EDGE
            return a, 10
    if types[EXCHANGE]:
        give = legal_res(_head(masks, 9)[0])
        g = _argbest(give, lambda r: (hand[r],))
        if g is not None and hand[g] >= 5:
            a[0], a[15] = EXCHANGE, g
            a[16] = _argbest(legal_res(_head(masks, 10)), lambda r: (-hand[r],)) or 0
            return a, 11
    if types[ENDTURN]:
        a[0] = ENDTURN
        return a, 12
    # the fall-back: the lowest legal type but ProposeTrade, sub-heads at their lowest legal index
    t = _lowest([types[k] and k != PROPOSE for k in range(13)])
    a[0] = t
    if t == SETTLE:
        a[1] = _lowest(_head(masks, 1)[0])
    elif t == CITY:
        a[1] = _lowest(_head(masks, 1)[1])
    elif t == ROAD:
        a[2] = _lowest(_head(masks, 2))
    elif t == ROBBER:
        a[3] = _lowest(_head(masks, 3))
    elif t == PLAYDEV:
        a[4] = _lowest(_head(masks, 4))
        if a[4] == MONOPOLY:
            a[15] = _lowest(_head(masks, 9)[2])
        elif a[4] == YEAR_OF_PLENTY:
            a[15], a[16] = _lowest(_head(masks, 9)[3]), _lowest(_head(masks, 10))
    elif t == EXCHANGE:
        a[15], a[16] = _lowest(_head(masks, 9)[0]), _lowest(_head(masks, 10))
    elif t == RESPOND:
        a[5] = _lowest(_head(masks, 5))
    elif t == STEAL:
        a[6] = _lowest(_head(masks, 6)[1])
    elif t == DISCARD:
        a[17] = _lowest(_head(masks, 11))
    return a, 13


def decide_all(blobs, masks):
    """-> (actions int32 [n,18], rows int [n])"""
    out = [decide(b, m) for b, m in zip(np.asarray(blobs), np.asarray(masks))]
    return np.stack([a for a, _ in out]), np.array([r for _, r in out])
