"""The launch sequence of a `rocprofv3 --kernel-trace --memory-copy-trace --output-format csv` run as diff-able text: per queue (numbered
in order of first use) the kernel names in launch order (the first 60 characters and a hash of the full name; consecutive repeats folded into
`name xK`), the number of memory copies per direction, and the full name behind every hash.  usage: kernel_sequence.py OUTPUT_DIRECTORY_OF_ROCPROFV3"""
import collections
import csv
import glob
import hashlib
import os
import sys


def rows(pattern):
    for path in sorted(glob.glob(os.path.join(sys.argv[1], "**", pattern), recursive=True)):
        with open(path, newline="") as f:
            yield from csv.DictReader(f)


queues, legend = collections.OrderedDict(), {}
for r in sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"])):
    label = f'{r["Kernel_Name"][:60]} #{hashlib.sha1(r["Kernel_Name"].encode()).hexdigest()[:6]}'
    legend[label] = r["Kernel_Name"]
    queues.setdefault(r["Queue_Id"], []).append(label)
for q, names in enumerate(queues.values()):
    print(f"queue {q}: {len(names)} launches")
    i = 0
    while i < len(names):
        j = i
        while j < len(names) and names[j] == names[i]:
            j += 1
        print(f"  {names[i]}" + (f" x{j - i}" if j - i > 1 else ""))
        i = j
for direction, k in sorted(collections.Counter(r["Direction"] for r in rows("*memory_copy_trace.csv")).items()):
    print(f"memory copies {direction}: {k}")
for label in sorted(legend):
    print(f"{label[-7:]} = {legend[label]}")
