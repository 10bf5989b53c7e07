#!/bin/bash
# What does the attention core (k_attn3h<8, true, false>, B = 64, E = 256, L = 1024) wait for?  Counter-only rocprofv3 passes (no
# tracing in the same run) over tools/attn_core_one.py, run inside TREE with that tree's library, reduced by tools/attn_core_pmc.py.
#   tools/attn_core_pmc.sh TREE OUTDIR        e.g.  tools/attn_core_pmc.sh ab_parent out/pmc_parent
R=$PWD; T=$1; O=$R/$2; rm -rf $O; mkdir -p $O
P=(
 "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE"
 "SQ_VALU_MFMA_BUSY_CYCLES SQ_VALU_MFMA_COEXEC_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_CMD_FIFO_FULL SQ_LDS_DATA_FIFO_FULL SQ_ACTIVE_INST_MISC GRBM_GUI_ACTIVE"
 "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_INST_CYCLES_VMEM_RD SQ_INST_LEVEL_VMEM GRBM_GUI_ACTIVE"
)
cd $R/$T || exit 1
for i in "${!P[@]}"; do
  timeout -k 10 150 rocprofv3 --pmc ${P[$i]} --output-format csv -d $O/p$i -o c -- python3 $R/tools/attn_core_one.py 64 256 1024 1 images 10 > $O/p$i.log 2>&1
  rc=$?; echo "pass $i rc=$rc"; tail -n 2 $O/p$i.log
  if [ $rc -ne 0 ]; then echo "pass $i failed: stopping"; exit $rc; fi
done
cd $R && python3 tools/attn_core_pmc.py $O | tee $O/summary.txt
