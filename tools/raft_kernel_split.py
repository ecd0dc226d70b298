"""Per-launch split of one RAFT update iteration from a kernel trace (MEASUREMENTS.md Part J).

    rocprofv3 --kernel-trace --stats -d <dir> -o raft --output-format csv -- \\
        python tools/raft_bench.py --skip_torch --sizes 768x432 --rounds 3 --capacity 2
    python tools/raft_kernel_split.py <dir>

An iteration of af_raft_flow is always the same 14 launches in the same order (raft.hip, run_iteration), so the dispatches of a flow
call can be named by their position: the trace is sorted by start time, every run of 20 k_lookup dispatches exactly 14 launches apart
is one flow call of 20 iterations, and each slot's time is averaged over the 20 iterations of that call.  Printed for the last flow
call of the trace at each batch size found (M = directions x grid positions differs, the launch sequence does not): mean time per
launch, share of the iteration's kernel time, and the wall span of the 280 launches against the sum of their kernel times (the
difference is launch gaps)."""
import collections
import csv
import glob
import os
import sys

SLOTS = ["k_lookup", "k_flow", "convc1 1x1 324>256", "convc2 3x3 256>192", "convf1 7x7 2>128", "convf2 3x3 128>64", "conv 3x3 256>126",
         "gru z|r 1x5 384>256", "gru q 1x5 384>128", "gru z|r 5x1 384>256", "gru q 5x1 384>128", "flow head 3x3 128>256", "flow head 3x3 256>2", "k_axpy1"]


def main():
    d = sys.argv[1] if len(sys.argv) > 1 else "."
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    k = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Grid_Size_X", r.get("Grid_Size", "?"))) for r in rows]
    idx = [i for i, r in enumerate(k) if r[0].startswith("k_lookup") or "k_lookup" in r[0][:40]]
    runs, i = [], 0
    while i < len(idx):
        j = i
        while j + 1 < len(idx) and idx[j + 1] - idx[j] == len(SLOTS):
            j += 1
        if j - i + 1 == 20:
            runs.append(idx[i])
        i = j + 1
    print("flow calls of 20 iterations in the trace:", len(runs))
    last = collections.OrderedDict()
    for s in runs:                      # the last call per lookup grid size = per batch size
        last[k[s][3]] = s
    for grid, start in last.items():
        acc = [0.0] * len(SLOTS)
        for it in range(20):
            for s in range(len(SLOTS)):
                r = k[start + len(SLOTS) * it + s]
                acc[s] += (r[2] - r[1]) / 1e3
        tot = sum(acc)
        span = (k[start + 20 * len(SLOTS) - 1][2] - k[start][1]) / 1e3
        print("== flow call with k_lookup grid %s: iteration = %.1f us of kernel time; 280 launches span %.1f us, kernels %.1f us" % (grid, tot / 20, span, tot))
        for s, n in enumerate(SLOTS):
            print("%-24s %8.1f us  %5.1f %%   %s" % (n, acc[s] / 20, 100 * acc[s] / tot, k[start + s][0][:48]))


if __name__ == "__main__":
    main()
