# end-of-round set: the whole GPU suite, the bench line with the driver's
# command (--steps 20 --warmup 5) and every leg (--full) with its CPU
# baseline curve, a kernel trace of the same command summarised into
# profiles/r04_<tag>_*; the PMC passes
# (tools/gpu_pmc.sh at 262,144 and 32,768 channels) are a separate call
#   bash tools/gpu_final.sh <tag>          (results under $MELPE_OUT/<tag>, default prof_out/<tag>)
cd "$(dirname "$0")/.." && O=${MELPE_OUT:-prof_out}/$1 && mkdir -p $O/profiles && export TMPDIR=/tmp &&
timeout -k 10 900 python -u -m pytest -s tests -x -v -m gpu --timeout 300 --timeout-method thread > $O/full_tests.log 2>&1 &&
timeout -k 10 900 python bench.py --full --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_kt -o kt -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/kt_bench.json 2> $O/kt_bench.err &&
python3 tools/prof_summary.py $O r04_$1 > $O/summary.log 2>&1 &&
cp profiles/r04_$1_* $O/profiles/
