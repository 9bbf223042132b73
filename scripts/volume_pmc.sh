#!/bin/bash
# Counters of k_volume_level (sdfhip_volume_build_device) on the 28 M-node scene's field, built to depth 8 from
# its 257^3 and from its 513^3 lattice: the same tree from two grids, the first at twice the second's time per node.  rocprofv3 --pmc
# alone, a few counters per pass (three TA counters in one pass are more than the profiler can place), one process per grid and pass;
# the summary is the mean per build over the level kernels' dispatches.
# usage: bash scripts/volume_pmc.sh [DIR]  (from the repository root; writes DIR/volume_pmc/ and DIR/volume_pmc.json; DIR: pmc_out)
ROOT=$(pwd); DIR=${1:-pmc_out}; case $DIR in /*) ;; *) DIR=$ROOT/$DIR;; esac; OUT=$DIR/volume_pmc; rm -rf $OUT; mkdir -p $OUT; export TMPDIR=/tmp
BUILDS=3
i=0
for pass in "GRBM_GUI_ACTIVE SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD" \
            "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum TCP_READ_TAGCONFLICT_STALL_CYCLES_sum" \
            "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA0_RDREQ_sum"; do
  i=$((i+1))
  for lattice in 8 9; do
    echo "pass $i lattice $lattice: $pass" >> $OUT/progress.txt
    timeout -k 5 150 rocprofv3 --pmc $pass --output-format csv -d $OUT/p${i}_l$lattice -- python3 scripts/volume_pmc.py --lattice $lattice --depth 8 --builds $BUILDS \
        > $OUT/p${i}_l$lattice.txt 2> $OUT/p${i}_l$lattice.err || { echo "pass $i lattice $lattice failed" >> $OUT/progress.txt; exit 1; }
  done
done
python3 scripts/volume_pmc.py --summarise $OUT --builds $BUILDS --out $DIR/volume_pmc.json
