"""numpy restatement of the action-row completion rule (include/catan_hip_tuning.h: catan_complete_action_rows) from the
float masks [325] and the deciding player's current_resources (obs_f[12:18]).  Uses no package code but `spec`.

A column that the row's action type does not use becomes the lowest legal index of the mask its head applies to the row (0 when that
mask is empty); `highest=True` takes the highest legal index instead - the joint log-prob of the row must not depend on which legal
value stands there, which is what the tests use it for."""
import numpy as np

from settlers_of_catan_rl_amd import spec

SETTLE, ROAD, CITY, BUYDEV, PLAYDEV, EXCHANGE, PROPOSE, RESPOND, ROBBER, ROLL, ENDTURN, STEAL, DISCARD = range(13)
YOP, MONO = 2, 4
MO, MS, MSHAPE = spec.MASK_OFFSETS, spec.MASK_SIZES, spec.MASK_SHAPES
# head -> the action column it fills (heads 7 / 8: the two trade lists, columns 7..10 and 11..14)
COLUMN = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 9: 15, 10: 16, 11: 17}


def head_mask(m, h):
    return (np.asarray(m[MO[h]:MO[h] + MS[h]]) > 0).reshape(MSHAPE[h])


def _pick(bits, highest):
    idx = np.flatnonzero(bits)
    return 0 if idx.size == 0 else int(idx[-1] if highest else idx[0])


def used_columns(row):
    """the columns of `row` that its type uses (never written by the completion); column 0 always"""
    t, card = int(row[0]), int(row[4])
    used = {0}
    if t in (SETTLE, CITY):
        used.add(1)
    if t == ROAD:
        used.add(2)
    if t == ROBBER:
        used.add(3)
    if t == PLAYDEV:
        used.add(4)
    if t == RESPOND:
        used.add(5)
    if t in (PROPOSE, STEAL):
        used.add(6)
    if t == EXCHANGE or (t == PLAYDEV and card in (YOP, MONO)):
        used.add(15)
    if t == EXCHANGE or (t == PLAYDEV and card == YOP):
        used.add(16)
    if t == DISCARD:
        used.add(17)
    if t == PROPOSE:
        used.update(range(7, 15))
    return used


def complete(row, m, res, highest=False):
    """row int [18], m float [325], res float [6] -> the completed row (a copy)"""
    a = np.array(row, copy=True)
    t = int(a[0])
    if t < 0 or t > 12:
        return a
    if t not in (SETTLE, CITY):
        a[1] = _pick(head_mask(m, 1)[2], highest)
    if t != ROAD:
        a[2] = _pick(head_mask(m, 2).reshape(-1), highest)
    if t != ROBBER:
        a[3] = _pick(head_mask(m, 3).reshape(-1), highest)
    if t != PLAYDEV:
        a[4] = _pick(head_mask(m, 4).reshape(-1), highest)
    if t != RESPOND:
        a[5] = _pick(head_mask(m, 5).reshape(-1), highest)
    if t not in (PROPOSE, STEAL):
        a[6] = _pick(head_mask(m, 6)[2], highest)
    card, m9 = int(a[4]), head_mask(m, 9)
    if not (t == EXCHANGE or (t == PLAYDEV and card in (YOP, MONO))):
        mt = m9[0 if t == EXCHANGE else 1]
        if t == PLAYDEV:
            mt = mt & m9[2 if card == MONO else (3 if card == YOP else 1)]
        a[15] = _pick(mt, highest)
    if not (t == EXCHANGE or (t == PLAYDEV and card == YOP)):
        a[16] = _pick(head_mask(m, 10).reshape(-1), highest)
    if t != DISCARD:
        a[17] = _pick(head_mask(m, 11).reshape(-1), highest)
    if t != PROPOSE:
        res = np.asarray(res)
        empty = float(res.sum()) == 0.0
        give = res > 0                    # head 7, first pick: the resources held; "stop" only with an empty hand
        give[0] = empty
        a[7] = _pick(give, highest)
        a[8:11] = 0
        a[11] = 0 if empty else (5 if highest else 1)     # head 8, first pick: every resource; "stop" only with an empty hand
        a[12:15] = 0
    return a


def complete_all(rows, masks, res, highest=False):
    return np.stack([complete(rows[i], masks[i], res[i], highest) for i in range(len(rows))])
