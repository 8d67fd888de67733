"""Per-kernel totals of a rocprofv3 rocpd database (`rocprofv3 --kernel-trace` without `--output-format csv` writes
<name>_results.db): python tools/rocpd_kernel_stats.py results.db out.csv -> Name, Calls, TotalDurationNs, AverageNs, Percentage,
MinNs, MaxNs, the columns of the tool's own kernel_stats.csv."""
import csv
import sqlite3
import sys


def main(db_path, out_path):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), sum(end - start), min(end - start), max(end - start) from kernels group by name order by 3 desc").fetchall()
    total = sum(r[2] for r in rows)
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
        for name, calls, dur, mn, mx in rows:
            w.writerow([name, calls, dur, round(dur / calls, 1), round(100.0 * dur / total, 3), mn, mx])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
