"""Harvests a start pool (settlers_of_catan_rl_amd/start_pool.py) from recorded games.

usage: make_start_pool.py RECORD.npz [RECORD.npz ...] -o pool.npz [--every K] [--keep-initial] [--min-turn T] [--max-turn T]
                          [--min-leader-vp V] [--max-leader-vp V] [--check]

Replays every record (record.replay: a one-game env on the GPU) and keeps the position behind every K-th action that passes the
filters; finished positions and duplicates are never kept.  Prints one summary line: entries, turn range, leader-VP histogram.
--check: the pool's blobs go through the state check (position.check_blobs) and a pool with an entry that breaks a rule is
not written: the entries and their rules are printed and the exit status is 1."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None, make_env=None, check=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("records", nargs="+", help="records saved by record.save")
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--keep-initial", action="store_true", help="also keep positions of the initial placement phase")
    ap.add_argument("--min-turn", type=int)
    ap.add_argument("--max-turn", type=int)
    ap.add_argument("--min-leader-vp", type=int)
    ap.add_argument("--max-leader-vp", type=int)
    ap.add_argument("--check", action="store_true", help="refuse to write a pool with an entry that breaks a state rule")
    a = ap.parse_args(argv)
    from settlers_of_catan_rl_amd import record, start_pool
    pool = start_pool.StartPool.from_records((record.load(p) for p in a.records), every=a.every, skip_initial=not a.keep_initial,
                                             min_turn=a.min_turn, max_turn=a.max_turn, min_leader_vp=a.min_leader_vp,
                                             max_leader_vp=a.max_leader_vp, make_env=make_env)
    if a.check:
        from settlers_of_catan_rl_amd import position
        viol = (check or position.check_blobs)(pool.blobs)
        viol = viol.cpu().numpy() if hasattr(viol, "cpu") else viol
        if (viol != 0).any():
            print(f"{a.out}: not written: {position.describe_bad(viol, limit=20)}")
            return 1
    start_pool.save(pool, a.out)
    print(f"{a.out}: {pool.summary()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
