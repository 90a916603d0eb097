"""Effective shader clock per kernel from a rocprofv3 --pmc GRBM_GUI_ACTIVE run (MI355X_MICROARCH.md, DVFS give-back):
  rocprofv3 --pmc GRBM_GUI_ACTIVE -d out --output-format csv -- python3 <script>
  python tools/pmc_clock.py out
clock = GRBM_GUI_ACTIVE / 8 XCDs / dispatch wall time (the csv's End_Timestamp - Start_Timestamp). The quotient reads high on
dispatches shorter than about 0.3 ms; profiled passes clock lower than plain ones, so compare profiled with profiled only."""
import collections
import csv
import glob
import sys

f = (glob.glob(sys.argv[1] + "/*/*counter_collection.csv") + glob.glob(sys.argv[1] + "/*counter_collection.csv"))[0]
acc = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    if r["Counter_Name"] != "GRBM_GUI_ACTIVE":
        continue
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
    short = name.split("(")[0].split("::")[-1][:40] + (" " + name[name.find("<"):name.find(">") + 1][:34] if "<" in name else "")
    ns = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
    if ns > 0:
        acc[short].append((ns, float(r["Counter_Value"]) / 8.0 / ns))
print("%-60s %6s %10s %10s %10s" % ("kernel", "calls", "avg ms", "clock GHz", "min..max"))
for k, v in sorted(acc.items(), key=lambda kv: -sum(x[0] for x in kv[1]))[:int(sys.argv[2]) if len(sys.argv) > 2 else 12]:
    ghz = sorted(x[1] for x in v)
    print("%-60s %6d %10.3f %10.3f %5.3f..%5.3f" % (k, len(v), sum(x[0] for x in v) / len(v) * 1e-6, ghz[len(ghz) // 2], ghz[0], ghz[-1]))
