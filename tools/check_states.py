"""Checks the state blobs of files against the state rules (include/catan_hip_tuning.h catan_state_check) on the device.

usage: check_states.py FILE.npz [FILE.npz ...] [--limit K]

Reads game records (record.save: start_blob, final_blob), start pools (start_pool.save: blobs) and plain .npz files: every integer array
whose last axis has 736 words is a list of blobs.  Prints one line per array and one per entry that breaks a rule, with the rules' names
(at most K per array, default 20).  Exit status 1 if any entry breaks a rule, 2 for a file without blobs, else 0.
The rules are necessary, not sufficient: an entry that passes need not be reachable by legal play."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def blob_arrays(path):
    """-> [(key, int32 [m, 736])] of one .npz"""
    import numpy as np
    from settlers_of_catan_rl_amd import spec
    out = []
    with np.load(path, allow_pickle=False) as z:
        for key in z.files:
            a = z[key]
            if a.dtype.kind in "iu" and a.ndim >= 1 and a.shape[-1] == spec.STATE_WORDS and a.size:
                out.append((key, a.reshape(-1, spec.STATE_WORDS).astype(np.int32)))
    return out


def main(argv=None, check=None):
    """check: blobs [m, 736] -> uint64 [m] (default: position.check_blobs on the current device)"""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+")
    ap.add_argument("--limit", type=int, default=20, help="entries named per array")
    a = ap.parse_args(argv)
    import numpy as np
    from settlers_of_catan_rl_amd import position
    if check is None:
        check = lambda blobs: position.check_blobs(blobs).cpu().numpy()
    status = 0
    for path in a.files:
        arrays = blob_arrays(path)
        if not arrays:
            print(f"{path}: no array of {736}-word blobs")
            status = max(status, 2)
        for key, blobs in arrays:
            v = np.asarray(check(blobs)).astype(np.uint64)
            bad = np.flatnonzero(v != 0)
            print(f"{path}:{key}: {len(blobs)} entries, {len(bad)} break a rule")
            for i in bad[:a.limit]:
                print(f"  entry {int(i)}: {', '.join(position.explain(v[i]))}")
            if len(bad) > a.limit:
                print(f"  ... and {len(bad) - a.limit} more")
            if len(bad):
                status = max(status, 1)
    return status


if __name__ == "__main__":
    sys.exit(main())
