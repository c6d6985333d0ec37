# usage (on an MI355X, from the repository root): bash tools/pmc_fit_verts.sh <output directory> [hand pairs, default 256] [iters, default 30]
# Two rocprofv3 --pmc passes (counters only, no tracing) over three launches of the vertex fit (tools/bench_fit_verts.py --only
# kernel), each pass under its own time limit; the second pass runs only if the first ended well.  Prints the counters of
# mano_fit_verts_kernel per dispatch.
set -o pipefail
export TMPDIR=/tmp
R=$(pwd); mkdir -p "$1"; O=$(cd "$1" && pwd)
A="SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY"
B="SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_VMEM"
cd /tmp
timeout -k 10 ${4:-240} rocprofv3 --pmc $A --output-format csv -d $O/a -o a -- python3 $R/tools/bench_fit_verts.py --only kernel --hands ${2:-256} --iters ${3:-30} > $O/a.out 2> $O/a.err &&
timeout -k 10 ${4:-240} rocprofv3 --pmc $B --output-format csv -d $O/b -o b -- python3 $R/tools/bench_fit_verts.py --only kernel --hands ${2:-256} --iters ${3:-30} > $O/b.out 2> $O/b.err
rc=$?
cd $R
echo "passes rc $rc"
[ $rc -eq 0 ] || { tail -5 $O/a.err $O/b.err 2>/dev/null; exit $rc; }
python3 - $O <<'PY'
import collections, csv, glob, sys
for d in ("a", "b"):
    for fn in glob.glob(sys.argv[1] + "/%s/**/*counter_collection.csv" % d, recursive=True):
        acc, n = collections.defaultdict(float), set()
        for r in csv.DictReader(open(fn)):
            if "mano_fit_verts" in r["Kernel_Name"]:
                acc[r["Counter_Name"]] += float(r["Counter_Value"])
                n.add(r["Dispatch_Id"])
        print(d, len(n), "dispatches", {k: "%.4g" % (v / max(len(n), 1)) for k, v in sorted(acc.items())})
PY
