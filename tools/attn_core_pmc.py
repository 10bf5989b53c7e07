"""Reduce the counter-only rocprofv3 passes over tools/attn_core_one.py (tools/attn_core_pmc.sh): the mean of every counter over
the last launches of k_attn3h, and the ratios that say what the attention core waits for.
    python tools/attn_core_pmc.py <directory with p*/ pass outputs> [launches, default 8]"""
import csv
import glob
import re
import sys
from collections import defaultdict

root, last = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8
vals, dur = defaultdict(lambda: defaultdict(list)), defaultdict(list)
for f in sorted(glob.glob(root + "/p*/**/*counter_collection.csv", recursive=True)):
    per, meta = defaultdict(lambda: defaultdict(float)), {}
    for r in csv.DictReader(open(f)):
        m = re.search(r"k_attn3h<[^>]*>", r["Kernel_Name"])
        if not m:
            continue
        d = int(r["Dispatch_Id"])
        per[d][r["Counter_Name"]] += float(r["Counter_Value"])
        meta[d] = (m.group(0) + f" grid={r['Grid_Size']} vgpr={r.get('VGPR_Count', '?')}+{r.get('Accum_VGPR_Count', '?')} "
                   f"lds={r.get('LDS_Block_Size', '?')} scratch={r.get('Scratch_Size', '?')}",
                   (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 if r.get("End_Timestamp") else 0.0)
    by_k = defaultdict(list)
    for d in sorted(per):
        by_k[meta[d][0]].append(d)
    for k, ds in by_k.items():
        for d in ds[-last:]:
            for c, v in per[d].items():
                vals[k][c].append(v)
            dur[k].append(meta[d][1])
for k in sorted(vals):
    c = {n: sum(v) / len(v) for n, v in vals[k].items()}
    us = sum(dur[k]) / len(dur[k])
    print(f"\n== {k}   {us:.1f} us under the profiler")
    for n in sorted(c):
        print(f"   {n:36s} {c[n]:16.0f}")
    g = c.get("GRBM_GUI_ACTIVE", 0) / 8.0            # cycles of the launch (summed over the 8 XCDs)
    wc = c.get("SQ_WAVE_CYCLES", 0)
    if g and us:
        print(f"   -> clock {g / us / 1e3:.2f} GHz, {g:.0f} cycles per launch")
    if g and wc and "SQ_WAIT_ANY" in c:
        print(f"   -> wave-cycle shares: s_waitcnt / s_barrier {c['SQ_WAIT_ANY'] / wc:.2f}, issue-stalled {c['SQ_WAIT_INST_ANY'] / wc:.2f} "
              f"(of which LDS {c['SQ_WAIT_INST_LDS'] / wc:.2f}); busy issuing: VALU (matrix included) {c['SQ_ACTIVE_INST_VALU'] / wc:.2f} "
              f"VMEM {c['SQ_ACTIVE_INST_VMEM'] / wc:.2f} LDS {c['SQ_ACTIVE_INST_LDS'] / wc:.2f}")
    if g and "SQ_VALU_MFMA_BUSY_CYCLES" in c:
        print(f"   -> matrix pipe busy {c['SQ_VALU_MFMA_BUSY_CYCLES'] / 1024 / g:.3f} of the launch, vector + matrix co-executing "
              f"{c.get('SQ_VALU_MFMA_COEXEC_CYCLES', 0) / 1024 / g:.3f}")
    if g and "SQ_LDS_IDX_ACTIVE" in c:
        print(f"   -> LDS array busy {c['SQ_LDS_IDX_ACTIVE'] / 256 / g:.3f} of the launch per CU, bank-conflict cycles "
              f"{c.get('SQ_LDS_BANK_CONFLICT', 0) / 256 / g:.3f}")
    if g and "SQ_INSTS_VALU" in c:
        print(f"   -> instructions per wave: VALU (matrix included) {c['SQ_INSTS_VALU'] / c['SQ_WAVES']:.0f}, matrix "
              f"{c.get('SQ_INSTS_MFMA', 0) / c['SQ_WAVES']:.0f}, LDS {c['SQ_INSTS_LDS'] / c['SQ_WAVES']:.0f}, "
              f"SALU {c['SQ_INSTS_SALU'] / c['SQ_WAVES']:.0f}")
