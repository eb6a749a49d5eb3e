"""Regenerates tests/golden/mpc_profit_sums.json.  Run in the BUILD container only (`python tests/golden/make_mpc_sums.py`): it
reads the MPC benchmark's result files the reference holds (data files, SHEMS python/single_building/results/); nothing on a GPU box
reads them.  Only numbers go into the fixture: per result file, keyed "ChargerNN_split" as tables.real_series_keys(),
    rows           the row count (one row per MPC decision)
    profits_sum    the sum of the `profits` column
    ext_ev_sum     the sum of the `EXT_EV` column
    profit_total   what the MPC scored on the file's horizon (see profits_is)
    profits_is     how `profits` is to be read.  The reference's writer (run_SHEMS.py:57-73) stores `results` as the optimiser built
                   it, and the optimiser (SHEMS_optimizer_cost.py:92-97) puts ONE number -- the sum over the control horizon of
                   p_sell * PV_GR - p_buy * (GR_DE + GR_EV) -- into the `profits` cell of EVERY row.  So the column is neither per
                   hour nor a running total: "total_repeated" when every row holds the same value (profits_sum = rows * profit_total),
                   otherwise "per_hour" or "running_total" as the column itself shows.
"""
import csv
import glob
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = "/root/reference/SHEMS python/single_building/results"


def read(path):
    rows = list(csv.DictReader(open(path)))
    prof = [float(r["profits"]) for r in rows]
    ext = [float(r["EXT_EV"]) for r in rows]
    if all(p == prof[0] for p in prof):
        kind, total = "total_repeated", prof[0]
    elif all(b >= a for a, b in zip(prof, prof[1:])) or all(b <= a for a, b in zip(prof, prof[1:])):
        kind, total = "running_total", prof[-1]
    else:
        kind, total = "per_hour", sum(prof)
    return dict(rows=len(rows), profits_sum=sum(prof), ext_ev_sum=sum(ext), profit_total=total, profits_is=kind)


def main():
    out = {}
    for path in sorted(glob.glob(os.path.join(REF_DIR, "*_results_*_all_*_fix_Charger*.csv"))):
        m = re.search(r"_all_(train|eval|test)_fix_(Charger\d\d)\.csv$", path)
        out[f"{m.group(2)}_{m.group(1)}"] = read(path)
    with open(os.path.join(HERE, "mpc_profit_sums.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(len(out), "result files ->", os.path.join(HERE, "mpc_profit_sums.json"))


if __name__ == "__main__":
    main()
