"""Opponent league: the snapshot deque and its sampling rule (reference RL/ppo/update_opponent_policies.py:13-43 and the
bookkeeping around it in RL/robust_train.py:62-64,136-141).

The reference keeps up to `num_policies_to_store` (500) earlier state-dicts of the central policy, appends one every
`add_policy_every` (4) updates, and every `update_opponent_policies_every` (1) updates gives EACH WORKER PROCESS three
opponents drawn with `np.random.choice(earlier_policies, 3, p=p)`: p is half uniform, half linearly increasing over the
most recent `linear_num` (800) snapshots.  A worker hosts `num_envs_per_process` (5) games that share its three opponent
nets; inside a game the seat -> policy-slot map is fixed at start-up (game_manager.py:24-31).

Here the "workers" are consecutive groups of `envs_per_worker` games of the batched env.  `sample` reproduces the
reference draw exactly (same numpy generator calls, same order) and returns snapshot indices per worker; the collector
then runs one batched forward per DISTINCT net in play (rollout.RolloutCollector, grouped inference).  With 65 536 games
the exact rule would put up to 500 distinct nets in play - 500 small forwards per pass - so `max_distinct=K` offers a
bounded variant: K snapshots are drawn i.i.d. from p and every worker draws its three uniformly among those K (each
opponent is still marginally p-distributed; only the correlation between workers changes).  max_distinct=None is the
reference rule.

Results (no counterpart in the reference).  A collector built with league_stats=True leaves, after every rollout, a table of who won
the finished games per opponent net (csrc/catan_league_stats.hip).  `record` books those rows under the snapshots' SERIAL NUMBERS -
a snapshot keeps its number while it moves through the deque - and `central_share` turns them into the central policy's share of the
decided seats against each snapshot.  sampling="pfsp" (prioritised fictitious self-play) mixes the reference distribution with
weights (1 - share) ** power, so that the snapshots the central policy does badly against are drawn more often; sampling="reference",
the default, makes the reference's generator calls whatever has been recorded.
"""
import copy
from collections import deque

import numpy as np
import torch


def get_prob_dist(num_policies, linear_num=800, linear_prob=0.5):
    """update_opponent_policies.py:29-43: (1 - linear_prob) spread uniformly + a linear ramp over the last
    min(linear_num, num_policies) entries (ramp value i * grad for the i-th of them, so the oldest of them adds 0)."""
    p = np.full((num_policies,), (1.0 - linear_prob) / num_policies)
    num_aux = min(linear_num, num_policies)
    h = (2 * linear_prob) / (num_aux + 1)
    grad = h / num_aux
    p[num_policies - num_aux:] += np.arange(num_aux) * grad
    return p / np.sum(p)


class League(object):
    def __init__(self, num_policies_to_store=500, add_policy_every=4, update_opponent_policies_every=1, envs_per_worker=5,
                 max_distinct=None, seed=0, sampling="reference", pfsp_power=2.0, pfsp_mix=0.5, pfsp_prior=1.0, decay=0.9):
        """sampling: "reference" (the reference's draw) or "pfsp" (see `probabilities`).  pfsp_power, pfsp_mix, pfsp_prior (the `a` of
        `central_share`) and decay (every `record` first multiplies what is on record by it) are hyper-parameter defaults - power 2 is
        the usual PFSP choice -, not measured optima."""
        if sampling not in ("reference", "pfsp"):
            raise ValueError(f'sampling must be "reference" or "pfsp", got {sampling!r}')
        self.earlier = deque(maxlen=num_policies_to_store)                   # robust_train.py:62
        # `earlier` stays a plain deque of state-dicts (callers extend and clear it directly); the serial numbers live beside it and
        # are brought up to date lazily (`serials`): _known holds the very objects the numbers in _serials belong to
        self._serials, self._known, self._next_serial = [], [], 0
        self.records = {}                # serial -> float64 [6] (spec.LEAGUE_STATS_FIELDS), decayed sums
        self.in_play = None              # `assign`: the serials of the collector's nets, in its net order
        self.sampling, self.pfsp_power, self.pfsp_mix, self.pfsp_prior, self.decay = sampling, float(pfsp_power), float(pfsp_mix), float(pfsp_prior), float(decay)
        self.add_policy_every = add_policy_every
        self.update_every = update_opponent_policies_every
        self.envs_per_worker = envs_per_worker
        self.max_distinct = max_distinct
        self.rng = np.random.RandomState(seed)       # the reference uses numpy's global RandomState: same algorithm

    def add(self, policy):
        """robust_train.py:63-64,136-137: a CPU copy of the central policy's state-dict."""
        self.earlier.append({k: v.detach().to("cpu", copy=True) for k, v in policy.state_dict().items()})

    def after_update(self, update_num, policy):
        """robust_train.py:135-141, called once per PPO update with the 0-based update number: returns True when the
        opponents should be re-drawn."""
        if update_num % self.add_policy_every == 0 and update_num > 0:
            self.add(policy)
        return update_num % self.update_every == 0

    def serials(self):
        """-> the serial number of every entry of `earlier`, oldest first.  A snapshot gets the next free number when it is first seen
        here and keeps it until the deque drops it; the records of dropped snapshots go with them."""
        entries = list(self.earlier)
        if len(entries) != len(self._known) or any(a is not b for a, b in zip(entries, self._known)):
            have = {id(o): s for o, s in zip(self._known, self._serials)}
            out = []
            for o in entries:
                s = have.get(id(o))
                if s is None:
                    s, self._next_serial = self._next_serial, self._next_serial + 1
                out.append(s)
            self._serials, self._known = out, entries
            alive = set(out)
            self.records = {s: r for s, r in self.records.items() if s in alive}
        return list(self._serials)

    def restore(self, serials, records):
        """A checkpoint's serial numbers (for the entries now in `earlier`, oldest first) and records {serial: six numbers}."""
        serials = [int(s) for s in serials]
        if len(serials) != len(self.earlier):
            raise ValueError(f"{len(serials)} serial numbers for {len(self.earlier)} snapshots")
        self._serials, self._known = serials, list(self.earlier)
        self._next_serial = max(serials, default=-1) + 1
        self.records = {int(s): np.asarray(r, dtype=np.float64).reshape(6).copy() for s, r in records.items() if int(s) in set(serials)}
        self.in_play = None

    def record(self, table, reduce=None):
        """Books a rollout's league table (int64 [nets + 1, 6], storage.league_stats: a row per net of the last `assign`, in its order,
        then the totals row, which is not used here) under the snapshots' serial numbers.  Everything on record is first multiplied
        by `decay`.  reduce: a callable applied to the dense int64 tensor [len(earlier), 6] of this rollout's rows (in deque order)
        before it is added - a sum over ranks, so that every rank holds the same records.  Rows of snapshots the deque has dropped
        since the draw are dropped too."""
        if self.in_play is None:
            raise ValueError("League.record: no assignment on record (League.assign)")
        rows = torch.as_tensor(table).to(torch.int64).reshape(-1, 6)
        if rows.shape[0] != len(self.in_play) + 1:
            raise ValueError(f"League.record: a table of {len(self.in_play)} nets has {len(self.in_play) + 1} rows, got {rows.shape[0]}")
        serials = self.serials()
        pos = {s: i for i, s in enumerate(serials)}
        dense = torch.zeros((len(serials), 6), dtype=torch.int64)
        for k, s in enumerate(self.in_play):
            if s in pos:
                dense[pos[s]] += rows[k]
        if reduce is not None:
            dense = torch.as_tensor(reduce(dense)).to(torch.int64).cpu().reshape(len(serials), 6)
        for s in self.records:
            self.records[s] = self.records[s] * self.decay
        add = dense.numpy().astype(np.float64)
        for i, s in enumerate(serials):
            if add[i].any():
                self.records[s] = self.records.get(s, np.zeros(6, dtype=np.float64)) + add[i]

    def central_share(self):
        """-> float64 [len(earlier)]: per snapshot x = (central_wins + a) / (central_wins + net_wins + 2a), a = pfsp_prior: the central
        policy's share of the seats either of the two won.  0.5 for a snapshot never met (and for any with a = 0 and no decided seat)."""
        x = np.full(len(self.earlier), 0.5)
        for i, s in enumerate(self.serials()):
            r = self.records.get(s)
            if r is not None:
                den = r[3] + r[2] + 2.0 * self.pfsp_prior
                if den > 0:
                    x[i] = (r[3] + self.pfsp_prior) / den
        return x

    def probabilities(self):
        """-> the distribution the next draw uses.  "reference": get_prob_dist(n).  "pfsp": (1 - mix) * get_prob_dist(n) + mix * w / sum(w)
        with w = (1 - central_share) ** power, and get_prob_dist(n) in place of w / sum(w) where sum(w) == 0."""
        n = len(self.earlier)
        p = get_prob_dist(n)
        if self.sampling != "pfsp":
            return p
        w = (1.0 - self.central_share()) ** self.pfsp_power
        tot = float(np.sum(w))
        return (1.0 - self.pfsp_mix) * p + self.pfsp_mix * (w / tot if tot > 0 else p)

    def sample(self, num_workers):
        """-> int64 [num_workers, 3] snapshot indices into `self.earlier`."""
        n = len(self.earlier)
        p = self.probabilities()
        if self.max_distinct is None:
            return np.stack([self.rng.choice(n, 3, p=p) for _ in range(num_workers)]).astype(np.int64)
        pool = self.rng.choice(n, self.max_distinct, p=p)
        return pool[self.rng.randint(0, self.max_distinct, size=(num_workers, 3))].astype(np.int64)

    def assign(self, collector, make_net):
        """Draws opponents for every worker of `collector` and installs them: one net per distinct snapshot in play
        (`make_net()` builds an empty net on the collector's device), per-game opponent indices for the three opponent
        policy slots."""
        N = collector.N
        workers = -(-N // self.envs_per_worker)
        idx = self.sample(workers)                                           # [workers, 3] snapshot ids
        distinct, inv = np.unique(idx, return_inverse=True)
        inv = inv.reshape(idx.shape)
        nets = []
        for s in distinct:
            net = make_net()
            net.load_state_dict(self.earlier[int(s)])
            net.eval()
            nets.append(net)
        per_game = np.repeat(inv, self.envs_per_worker, axis=0)[:N]          # games of a worker share its opponents
        serials = self.serials()
        self.in_play = [serials[int(s)] for s in distinct]
        collector.set_opponents(nets, torch.from_numpy(per_game))
        return distinct
