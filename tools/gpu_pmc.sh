# kernel trace + PMC passes of the encode/decode step at one channel count
# (one counter group per pass, each its own run and time limit), summarised
# into profiles/r04_<tag>_* and merged into profiles/pmc_latest.json (one
# set per channel count), copied to $MELPE_OUT/<tag>/profiles (default
# prof_out/<tag>/profiles)
#   bash tools/gpu_pmc.sh <tag> <channels>
cd "$(dirname "$0")/.." && O=${MELPE_OUT:-prof_out}/$1 && mkdir -p $O/profiles && export TMPDIR=/tmp &&
C=$2 &&
B="bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-side-legs --total-channels 0 --tx-channels 0 --rt-channels 0 --channels $C" &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof_kt -o kt -- python3 bench.py --full --no-cpu-baseline --no-side-legs --total-channels 0 --tx-channels 0 --rt-channels 0 --channels $C --steps 4 > $O/prof_kt.log 2>&1 &&
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch -o f -- python3 $B > $O/pmc_fetch.log 2>&1 &&
timeout -s KILL 300 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write -o w -- python3 $B > $O/pmc_write.log 2>&1 &&
timeout -s KILL 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_FLAT GRBM_GUI_ACTIVE -d $O/pmc_a -o a -- python3 $B > $O/pmc_a.log 2>&1 &&
timeout -s KILL 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY -d $O/pmc_b -o b -- python3 $B > $O/pmc_b.log 2>&1 &&
timeout -s KILL 300 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum -d $O/pmc_c -o c -- python3 $B > $O/pmc_c.log 2>&1 &&
python3 tools/prof_summary.py $O r04_$1 $C > $O/summary.log 2>&1 &&
cp profiles/r04_$1_* profiles/pmc_latest.json $O/profiles/ &&
rm -rf $O/pmc_fetch $O/pmc_write $O/pmc_a $O/pmc_b $O/pmc_c
