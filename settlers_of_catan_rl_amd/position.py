"""Positions written down: the state check of a blob (include/catan_hip_tuning.h catan_state_check) and `Position`, a
named, editable form of one 736-word state blob whose helpers keep the bookkeeping straight.

    mask = position.check_blobs(blobs, device)      # uint64 [cnt] on the device, bit r = rule spec.STATE_CHECK_RULES[r] is broken
    position.explain(int(mask[0]))                  # -> ["resource_conservation", ...]

    p = Position.blank()                            # the default board after the initial phase, nothing built, player 1 to roll
    p.settle(1, 0); p.road(1, 4); p.give(1, 3, 3); p.to_move(1, rolled=True, dice=(3, 4))
    env.import_state(p.to_blob(), [0], check=True)

The rules are necessary, not sufficient: a position that passes need not be reachable by legal play.
"""
import os

import numpy as np

from . import spec

_TOPOLOGY = None


def explain(mask):
    """a violation word -> the names of the rules it has set, in bit order"""
    m = int(mask)
    if m >> len(spec.STATE_CHECK_RULES):
        raise ValueError(f"violation word {m:#x} has bits beyond the {len(spec.STATE_CHECK_RULES)} rules")
    return [name for r, name in enumerate(spec.STATE_CHECK_RULES) if (m >> r) & 1]


def _device_blobs(blobs, device):
    """-> int32 device tensor [cnt, 736]"""
    import torch
    b = blobs if torch.is_tensor(blobs) else torch.from_numpy(np.array(blobs, dtype=np.int32))
    b = b.to(device=device, dtype=torch.int32)
    if b.dim() == 1:
        b = b[None]
    if b.dim() != 2 or b.shape[1] != spec.STATE_WORDS:
        raise ValueError(f"state blobs: shape [cnt, {spec.STATE_WORDS}] expected, got {tuple(b.shape)}")
    return b


def check_transposed(bt, want_count=False):
    """bt: int32 device tensor [736, cnt], contiguous (the orientation of catan_state_import) -> uint64 [cnt] device tensor of violation
    words; want_count: -> (words, number of blobs with a violation), which costs one 8-byte read (and waits for the stream)"""
    import torch
    from . import _lib
    from .env import _ptr, _stream
    L = _lib.lib()
    if not hasattr(L, "catan_state_check"):
        raise _lib.CatanHipError("the loaded library has no catan_state_check")
    if int(L.catan_state_check_rules()) != len(spec.STATE_CHECK_RULES):
        raise _lib.CatanHipError("the library's state-check rules are not spec.STATE_CHECK_RULES")
    cnt = int(bt.shape[1])
    if not bt.is_contiguous() or bt.dtype != torch.int32 or bt.shape[0] != spec.STATE_WORDS:
        raise ValueError("check_transposed: a contiguous int32 [736, cnt] tensor expected")
    with torch.cuda.device(bt.device):
        viol = torch.zeros((cnt,), dtype=torch.int64, device=bt.device)
        n_bad = torch.zeros((1,), dtype=torch.int64, device=bt.device) if want_count else None
        _lib.check(L.catan_state_check(_ptr(bt), cnt, _ptr(viol), _ptr(n_bad), _stream()))
        out = viol.view(torch.uint64)
        return (out, int(n_bad.item())) if want_count else out


def check_blobs(blobs, device=None):
    """blobs: [cnt, 736] (or one [736]), numpy or tensor, the orientation of export_state -> uint64 [cnt] device tensor: bit r set where
    the blob breaks rule spec.STATE_CHECK_RULES[r] (`explain`).  Only reads the blobs."""
    import torch
    if device is None:
        device = blobs.device if torch.is_tensor(blobs) and blobs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    b = _device_blobs(blobs, device)
    return check_transposed(b.t().contiguous())


def describe_bad(viol, limit=8):
    """uint64 violation words (tensor or array) -> 'blob 3: army, victory_points; blob 9: ...' for the first `limit` bad blobs"""
    v = viol.cpu().numpy() if hasattr(viol, "cpu") else np.asarray(viol)
    v = v.view(np.uint64) if v.dtype == np.int64 else v.astype(np.uint64)
    bad = np.flatnonzero(v != 0)
    parts = [f"blob {int(i)}: {', '.join(explain(v[i]))}" for i in bad[:limit]]
    more = f" (and {len(bad) - limit} more)" if len(bad) > limit else ""
    return f"{len(bad)} of {len(v)} blobs break the state rules: " + "; ".join(parts) + more


def require_legal(bt, what):
    """raises ValueError naming the first eight bad blobs of bt (int32 device [736, cnt]) and their rules; one launch, one 8-byte read"""
    viol, n_bad = check_transposed(bt, want_count=True)
    if n_bad:
        raise ValueError(f"{what}: {describe_bad(viol)}")


def topology():
    """edge_corner [72, 2], corner_nbr [54, 3] (-1: none), harbour_slot_corner [9, 2]: parsed once from csrc/catan_topology.inc"""
    global _TOPOLOGY
    if _TOPOLOGY is None:
        import re
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "catan_topology.inc")) as f:
            text = f.read()

        def table(name):
            body = re.search(name + r"(?:\[\d+\])+ = \{(.*?)\};", text, re.S).group(1)
            return np.array([int(x) for x in re.findall(r"\d+", body)], dtype=np.int64)
        nbr = table("CORNER_NBR_C").reshape(54, 3)
        slot_of = table("CORNER_HSLOT")
        slots = np.array([np.flatnonzero(slot_of == s) for s in range(9)], dtype=np.int64)
        _TOPOLOGY = {"edge_corner": table("EDGE_CORNER").reshape(72, 2), "corner_nbr": np.where(nbr == 255, -1, nbr),
                     "harbour_slot_corner": slots}
    return _TOPOLOGY


class Position(object):
    """One state blob by the names of spec.STATE_FIELDS: `p["p1_res"]` is an int32 array that may be edited in place, and to_blob() puts
    the words back where from_blob() found them (exact inverses on every blob, padding words included).

    The editing helpers change a position the way the game's bookkeeping would - a settlement comes out of the player's stock, a
    resource card out of the bank, a development card out of the pile - raise ValueError for what the rules of the state check forbid,
    and finish with refresh(), so that a legal position stays legal.  Player ids are 1..4, resources 1..5 (Brick, Wood, Ore, Sheep,
    Wheat), cards 0..4 (Knight, VictoryPoint, YearOfPlenty, RoadBuilding, Monopoly)."""

    def __init__(self, fields):
        self.f = fields

    # ---- blob <-> names
    @classmethod
    def from_blob(cls, blob):
        b = blob.detach().cpu().numpy() if hasattr(blob, "detach") else np.asarray(blob)
        b = b.reshape(-1)
        if b.shape[0] != spec.STATE_WORDS:
            raise ValueError(f"a state blob has {spec.STATE_WORDS} words, got {b.shape[0]}")
        return cls({name: b[off:off + n].astype(np.int32) for name, (off, n) in spec.STATE_OFFSETS.items()})

    def to_blob(self):
        out = np.zeros(spec.STATE_WORDS, dtype=np.int32)
        for name, (off, n) in spec.STATE_OFFSETS.items():
            out[off:off + n] = self.f[name]
        return out

    @classmethod
    def from_env(cls, env, game):
        """game `game` of a VecCatanEnv, as it stands"""
        return cls.from_blob(env.export_state([int(game)])[0])

    @classmethod
    def blank(cls, tile_res=None, harbour_type=None, player_order=(1, 2, 3, 4)):
        """The position just after the initial phase with nothing on the board: every card in the bank and the pile, every piece in stock,
        the first player of `player_order` to roll.  tile_res: 19 terrains (default spec.TERRAIN_TO_PLACE), the tokens follow in
        spec.DEFAULT_NUMBER_ORDER along spec.NUMBER_PLACEMENT_INDS; harbour_type: the 9 harbour ids by slot (default 0..8)."""
        p = cls.from_blob(np.zeros(spec.STATE_WORDS, dtype=np.int32))
        res = list(spec.TERRAIN_TO_PLACE if tile_res is None else tile_res)
        spec.normalise_board_config({"fixed_terrain_placements": res})
        p["tile_res"][:] = res
        tokens = iter(spec.DEFAULT_NUMBER_ORDER)
        for t in spec.NUMBER_PLACEMENT_INDS:
            p["tile_val"][t] = 7 if res[t] == 0 else next(tokens)
        p["robber_tile"][0] = res.index(0)
        p["harbour_type"][:] = list(range(9)) if harbour_type is None else harbour_type
        for q in (1, 2, 3, 4):
            p[f"p{q}_hidden"][:] = -1
            p[f"p{q}_played"][:] = -1
        p["bank_res"][:] = spec.RESOURCE_CARDS_EACH
        p["settlements_left"][:] = 5
        p["cities_left"][:] = 4
        p["pile_len"][0] = 25
        p["pile"][:] = [c for c, k in enumerate(spec.DEV_CARD_COUNTS) for _ in range(k)]
        if sorted(player_order) != [1, 2, 3, 4]:
            raise ValueError("player_order is a permutation of 1..4")
        p["player_order"][:] = player_order
        p["players_go"][0] = player_order[0]
        p["init_settlements"][:] = 2
        p["init_roads"][:] = 2
        p["init_second_corner"][:] = -1
        return p

    def __getitem__(self, name):
        return self.f[name]

    def copy(self):
        return Position({k: v.copy() for k, v in self.f.items()})

    # ---- helpers
    @staticmethod
    def _pid(pid):
        if int(pid) not in (1, 2, 3, 4):
            raise ValueError(f"a player id is 1..4, got {pid}")
        return int(pid)

    def settle(self, pid, corner):
        pid, c, T = self._pid(pid), int(corner), topology()
        if not 0 <= c < 54 or self["corner_bld"][c] != 0:
            raise ValueError(f"corner {corner} is not a free corner")
        if any(n >= 0 and self["corner_bld"][n] != 0 for n in T["corner_nbr"][c]):
            raise ValueError(f"corner {c} neighbours a built corner (distance rule)")
        if self["settlements_left"][pid - 1] < 1:
            raise ValueError(f"player {pid} has no settlement left")
        self["corner_bld"][c], self["corner_owner"][c] = 1, pid
        self["settlements_left"][pid - 1] -= 1
        return self.refresh()

    def city(self, pid, corner):
        pid, c = self._pid(pid), int(corner)
        if not 0 <= c < 54 or self["corner_bld"][c] != 1 or self["corner_owner"][c] != pid:
            raise ValueError(f"player {pid} has no settlement on corner {corner}")
        if self["cities_left"][pid - 1] < 1:
            raise ValueError(f"player {pid} has no city left")
        self["corner_bld"][c] = 2
        self["cities_left"][pid - 1] -= 1
        self["settlements_left"][pid - 1] += 1
        return self.refresh()

    def road(self, pid, edge):
        pid, e, T = self._pid(pid), int(edge), topology()
        if not 0 <= e < 72 or self["edge_owner"][e] != 0:
            raise ValueError(f"edge {edge} is not a free edge")
        ends = T["edge_corner"][e]
        mine = np.flatnonzero(self["edge_owner"] == pid)
        if not any(self["corner_owner"][c] == pid or any(c in T["edge_corner"][m] for m in mine) for c in ends):
            raise ValueError(f"edge {e} touches neither a building nor a road of player {pid}")
        self["edge_owner"][e] = pid
        return self.refresh()

    def give(self, pid, resource, k=1):
        """k cards of Resource `resource` (1..5) from the bank to the player's hand, back to the bank for k < 0"""
        pid, r, k = self._pid(pid), int(resource) - 1, int(k)
        if not 0 <= r < 5:
            raise ValueError(f"a resource is 1..5, got {resource}")
        hand, vis = self[f"p{pid}_res"], self[f"p{pid}_vis"]
        if self["bank_res"][r] < k or hand[r] + k < 0:
            raise ValueError(f"give({pid}, {resource}, {k}): the bank holds {self['bank_res'][r]}, the hand {hand[r]}")
        self["bank_res"][r] -= k
        hand[r] += k
        vis[r] = min(max(vis[r] + k, 0), hand[r])
        return self.refresh()

    def deal_card(self, pid, card, played=False):
        """one development card `card` (0..4) out of the pile into the player's hidden cards, or among his played ones"""
        pid, card = self._pid(pid), int(card)
        n = int(self["pile_len"][0])
        where = [i for i in range(n) if self["pile"][i] == card]
        if not 0 <= card <= 4 or not where:
            raise ValueError(f"no card {card} is left in the pile")
        pile = [int(x) for x in self["pile"][:n]]
        del pile[where[-1]]
        self["pile"][:] = pile + [-1] * (25 - len(pile))
        self["pile_len"][0] = n - 1
        ln, lst = (f"p{pid}_n_played", f"p{pid}_played") if played else (f"p{pid}_n_hidden", f"p{pid}_hidden")
        self[lst][int(self[ln][0])] = card
        self[ln][0] += 1
        return self.refresh()

    def move_robber(self, tile):
        if not 0 <= int(tile) < 19:
            raise ValueError(f"a tile is 0..18, got {tile}")
        self["robber_tile"][0] = int(tile)
        return self

    def to_move(self, pid, rolled=False, dice=None):
        """it is player pid's go in the main phase, before (rolled=False) or after the roll; dice: the two dice of a rolled turn
        (default 3 and 4).  Whatever was pending - an offer, discards, a road-building card, cards bought this turn - is cleared."""
        pid = self._pid(pid)
        order = [int(x) for x in self["player_order"]]
        if pid not in order:
            raise ValueError(f"player {pid} is not in player_order {order}")
        if dice is not None and not (rolled and len(dice) == 2 and all(1 <= int(d) <= 6 for d in dice)):
            raise ValueError("dice are two values 1..6 of a rolled turn")
        self["players_go"][0], self["player_order_id"][0] = pid, order.index(pid)
        self["dice_rolled"][0] = int(bool(rolled))
        self["die1"][0], self["die2"][0] = (dice if dice is not None else (3, 4)) if rolled else (0, 0)
        for name in ("played_dev", "must_use_dev", "must_respond", "trade_proposer", "trade_target", "trade_n_give", "trade_give",
                     "trade_n_recv", "trade_recv", "road_building_active", "road_building_count", "can_move_robber", "just_moved_robber",
                     "need_discard", "n_to_discard", "to_discard", "trades_this_turn", "actions_this_turn", "bought_this_turn"):
            self[name][:] = 0
        return self

    # ---- what follows from the rest
    def refresh(self, env=None):
        """Recomputes the words that follow from the others: the harbour flags, cur_army_size, the two title holders, every player's
        victory points with curr_vps and winner, and the estimates, which are set to the exact hands.  With `env` (a VecCatanEnv, or any
        object with position_longest_paths(blob) -> four lengths) cur_longest_path is searched afresh on a one-game env of its own beside
        `env`, whose games are not touched; without it the four words stay.
        The holders: a present holder stays while he still ties for the lead at or above the title's least size (3 knights, 5 roads);
        otherwise the unique leader at or above it holds; otherwise nobody."""
        T = topology()
        ids = (1, 2, 3, 4)
        if env is not None:
            self["cur_longest_path"][:] = _longest_paths(env, self.to_blob())
        bld, own = self["corner_bld"], self["corner_owner"]
        for q in ids:
            flags = np.zeros(6, dtype=np.int32)
            for s in range(9):
                if any(bld[c] != 0 and own[c] == q for c in T["harbour_slot_corner"][s]):
                    flags[spec.HARBOUR_FLAG_OF_ID[int(self["harbour_type"][s])]] = 1
            self[f"p{q}_harbours"][:] = flags
            played = self[f"p{q}_played"][:int(self[f"p{q}_n_played"][0])]
            self["cur_army_size"][q - 1] = int((played == 0).sum())
        for who, count, sizes, least in (("la_player", "la_count", self["cur_army_size"], 3), ("lr_player", "lr_count", self["cur_longest_path"], 5)):
            top = int(sizes.max())
            h = int(self[who][0])
            if not (h in ids and sizes[h - 1] == top and top >= least):
                lead = np.flatnonzero(sizes == top)
                h = int(lead[0]) + 1 if top >= least and len(lead) == 1 else 0
            self[who][0], self[count][0] = h, (int(sizes[h - 1]) if h else 0)
        for q in ids:
            played = self[f"p{q}_played"][:int(self[f"p{q}_n_played"][0])]
            vp = int(((bld == 1) & (own == q)).sum()) + 2 * int(((bld == 2) & (own == q)).sum()) + int((played == 1).sum()) \
                + 2 * int(self["lr_player"][0] == q) + 2 * int(self["la_player"][0] == q)
            self[f"p{q}_vp"][0] = self["curr_vps"][q - 1] = vp
        go = int(self["players_go"][0])
        won = [q for q in ([go] + [q for q in ids if q != go]) if q in ids and self["curr_vps"][q - 1] >= 10]
        self["winner"][0] = won[0] if won else 0
        order = [int(x) for x in self["player_order"]]
        for q in ids:
            if q in order:
                for l in range(3):
                    hand = self[f"p{order[(order.index(q) + l + 1) % 4]}_res"]
                    self[f"p{q}_opp_min"][5 * l:5 * l + 5] = hand
                    self[f"p{q}_opp_max"][5 * l:5 * l + 5] = hand
        return self


def _longest_paths(env, blob):
    if hasattr(env, "position_longest_paths"):
        return [int(x) for x in env.position_longest_paths(blob)]
    import torch
    from .env import VecCatanEnv
    with torch.cuda.device(env.device):
        side = VecCatanEnv(1, device=env.device, auto_reset=False)
        side.import_state(blob)
        return [int(side.longest_path([q])[0]) for q in (1, 2, 3, 4)]
