"""LDS bank conflicts per kernel from one rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE pass:
    python tools/pmc_lds.py <dir given to rocprofv3 -d> [name filter]"""
import collections, csv, glob, subprocess, sys
cyc = collections.defaultdict(lambda: [0.0, 0.0])
for f in glob.glob(sys.argv[1] + "/**/*_counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = 0 if r["Counter_Name"] == "SQ_LDS_IDX_ACTIVE" else (1 if r["Counter_Name"] == "SQ_LDS_BANK_CONFLICT" else None)
        if k is not None:
            cyc[r["Kernel_Name"]][k] += float(r["Counter_Value"])
flt = sys.argv[2] if len(sys.argv) > 2 else ""
print("kernel | LDS-array cycles | bank-conflict cycles | %")
for name, (act, conf) in sorted(cyc.items(), key=lambda kv: -kv[1][0]):
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() if name.startswith("_Z") else name
    if flt in dem and act > 0:
        print(f"{dem:110s} {act:12.0f} {conf:12.0f} {100 * conf / act:5.1f}")
