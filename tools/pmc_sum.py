"""Sum rocprofv3 counter CSVs per counter over the k_stream dispatches:
    python tools/pmc_sum.py DIR [DIR ...]   (every *counter_collection.csv below each DIR)"""
import csv
import glob
import os
import sys

for d in sys.argv[1:]:
    tot, disp = {}, set()
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_stream" not in row["Kernel_Name"]:
                continue
            disp.add(row["Dispatch_Id"])
            tot[row["Counter_Name"]] = tot.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    print(f"{d}: {len(disp)} k_stream dispatches")
    for k in sorted(tot):
        print(f"  {k} {tot[k]:.0f}")
