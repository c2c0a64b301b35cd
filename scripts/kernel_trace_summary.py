"""Durations of chosen kernels in a rocprofv3 kernel trace, grouped by kernel and launch geometry: count, minimum, median and maximum in ns.

    rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -o cp -- python scripts/bench_count_penalty.py --batches 8,32 --rounds 1 --steps 32
    python scripts/kernel_trace_summary.py TRACE_DIR count_penalty logits_stats logits_finish > profiles/count_penalty_kernel_times.txt

Every *kernel_trace.csv under TRACE_DIR is read; a kernel is kept when its name contains one of the given substrings.  A line is
(kernel, Grid_Size_X, Grid_Size_Y, Workgroup_Size_X) -- grid sizes in threads, as the trace reports them -- then the figures.
"""
import csv
import glob
import statistics
import sys
from collections import defaultdict


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    wanted = sys.argv[2:]
    groups = defaultdict(list)
    for path in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                if not any(w in name for w in wanted):
                    continue
                key = (name.split("(")[0][-60:], row.get("Grid_Size_X"), row.get("Grid_Size_Y"), row.get("Workgroup_Size_X"))
                groups[key].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    for key, d in sorted(groups.items()):
        print(key, "n", len(d), "min_ns", min(d), "median_ns", int(statistics.median(d)), "max_ns", max(d))


if __name__ == "__main__":
    main()
