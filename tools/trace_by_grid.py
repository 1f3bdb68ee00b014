"""Group a rocprofv3 kernel trace by (kernel, grid): launches and median / min / max / total duration in us.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/text_bench.py --only attention
    python tools/trace_by_grid.py DIR [substring ...]      # only kernels whose name holds one of the substrings

Kernel names are cut to the function name and its template arguments; grids are in workgroups (x, y)."""
import csv
import glob
import json
import re
import statistics
import sys


def short(name: str) -> str:
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    m = re.match(r"[\w:]+(<[^()]*>)?", name)
    return (m.group(0) if m else name)[:96]


def main():
    rows = {}
    want = sys.argv[2:]
    for path in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(path)):
            name = short(r["Kernel_Name"])
            if want and not any(w in name for w in want):
                continue
            gx = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
            gy = int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"]))
            rows.setdefault((name, gx, gy), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, gx, gy), v in sorted(rows.items()):
        print(json.dumps({"kernel": name, "grid": [gx, gy], "launches": len(v),
                          "us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                          "us_max": round(max(v), 2), "us_total": round(sum(v), 1)}))


if __name__ == "__main__":
    main()
