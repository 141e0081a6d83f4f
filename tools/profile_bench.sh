#!/bin/bash
# Kernel trace + PMC passes of one bench.py configuration (run on the GPU box), one rocprofv3
# run per pass (kernel trace only beside --pmc; MI355X_MICROARCH.md rocprofv3 rules):
#   bash tools/profile_bench.sh <out_dir> <bench args...>
# Passes: trace (--kernel-trace --stats), fetch (FETCH_SIZE), write (WRITE_SIZE),
# tcc (TCC_HIT/MISS/EA0_RDREQ_128B), sq (SQ wave-cycle shares), f64 (f64 VALU instruction mix).
# Summarise afterwards with tools/pmc_traffic.py (key = bench.py's roofline.profile_key).
# PASSES="trace fetch" limits the run to those passes.
# Not in the default list: tcp (the L1's pending-miss stall and its L2 read requests) and tcplat
# (TCP_GATE_EN1, the requests' summed latency), DESIGN §5's k_h_eval counters.
# Per-XCC passes (not in the default list; tools/pmc_kernel_sum.py --per-xcc reads them): xtcc
# (TCC_HIT / TCC_MISS / TCC_EA0_RDREQ_128B) and xsq (SQ_BUSY_CYCLES / SQ_WAVES), each counter as
# eight derived counters <NAME>_xcc<k> = the sum over XCC k's instances, defined in
# <out_dir>/per_xcc.yaml (rocprofv3 -E).  FULL="" runs plain bench.py steps without --full.
set -eu
out=$1
shift
mkdir -p "$out"
export TMPDIR=/tmp
bench="python3 bench.py ${FULL---full --no-cpu-baseline} $*"
passes=${PASSES:-"trace fetch write tcc sq f64"}
xcc_counters="TCC_HIT TCC_MISS TCC_EA0_RDREQ_128B SQ_BUSY_CYCLES SQ_WAVES"
per_xcc_names() {  # the derived names of the given counters
    for c in "$@"; do for k in 0 1 2 3 4 5 6 7; do printf '%s_xcc%d ' "$c" $k; done; done
}
{
    printf 'rocprofiler-sdk:\n  counters-schema-version: 1\n  counters:\n'
    for c in $xcc_counters; do
        for k in 0 1 2 3 4 5 6 7; do
            printf '  - name: %s_xcc%d\n    description: %s summed over the instances of XCC %d\n' \
                "$c" $k "$c" $k
            printf '    properties: []\n    definitions:\n    - architectures:\n      - gfx950\n'
            printf '      expression: reduce(select(%s,[DIMENSION_XCC=[%d]]),sum)\n' "$c" $k
        done
    done
} > "$out/per_xcc.yaml"
for p in $passes; do
    case $p in
        tcp)   args="--pmc TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_sum" ;;
        tcplat) args="--pmc TCP_GATE_EN1_sum TCP_TCC_READ_REQ_LATENCY_sum" ;;
        xtcc)  args="-E $out/per_xcc.yaml --pmc $(per_xcc_names TCC_HIT TCC_MISS TCC_EA0_RDREQ_128B)" ;;
        xsq)   args="-E $out/per_xcc.yaml --pmc $(per_xcc_names SQ_BUSY_CYCLES SQ_WAVES)" ;;
        trace) args="--kernel-trace --stats" ;;
        fetch) args="--pmc FETCH_SIZE" ;;
        write) args="--pmc WRITE_SIZE" ;;
        tcc)   args="--pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_128B_sum" ;;
        sq)    args="--pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU" ;;
        f64)   args="--pmc SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_VMEM SQ_INSTS_SALU SQ_INSTS_LDS GRBM_GUI_ACTIVE" ;;
        *) echo "unknown pass $p"; exit 2 ;;
    esac
    echo "=== pass $p: rocprofv3 $args -- $bench"
    timeout -k 10 240 rocprofv3 $args -d "$out/$p" -o run --output-format csv -- $bench \
        > "$out/$p.log" 2>&1
    tail -n 1 "$out/$p.log"
done
