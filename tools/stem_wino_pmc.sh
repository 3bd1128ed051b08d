#!/bin/bash
# rocprofv3 counters of the stem + max-pool kernel in both forms (tools/stem_wino_probe.py --reps 5 --form ...),
# one pass per form; prints the last dispatch's counters summed over the chip.
#   tools/stem_wino_pmc.sh <output directory>
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(mkdir -p "${1:?usage: tools/stem_wino_pmc.sh <output directory>}" && cd "$1" && pwd)
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
pm="SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_MFMA SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE"
for form in direct wino; do
  timeout -k 10 150 rocprofv3 --kernel-trace --pmc $pm -d $out -o $form --output-format csv -- python $R/tools/stem_wino_probe.py --reps 5 --form $form > $out/$form.log 2>&1 || exit $?
done
python3 - <<PY
import csv, collections, glob
for f in sorted(glob.glob("$out/*_counter_collection.csv")):
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        if "conv_stem" in r["Kernel_Name"]:
            agg[r["Dispatch_Id"]][r["Counter_Name"]].append(float(r["Counter_Value"]))
    if not agg: continue
    last = sorted(agg, key=int)[-1]
    print(f.split("/")[-1], "dispatch", last)
    for k, v in sorted(agg[last].items()):
        print("   %-28s %.4g" % (k, sum(v)))
PY
