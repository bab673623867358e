#!/bin/bash
# One GPU-box pass: GPU tests, bench line, rocprofv3 kernel stats of the bench command.  Usage: tools/gpu_round.sh TAG [OUTDIR]
TAG=${1:-r02a}
O=${2:-results}
export TMPDIR=/tmp
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/${TAG}_pytest.log 2>&1; echo "pytest rc=$?" | tee -a $O/${TAG}_pytest.log
tail -3 $O/${TAG}_pytest.log
python bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err; echo "bench rc=$?"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${TAG}_prof -- python3 bench.py --full --no-cpu-baseline --no-secondary --reps 2 > $O/${TAG}_bench_prof.json 2> $O/${TAG}_bench_prof.err; echo "prof rc=$?"
head -c 1500 $O/${TAG}_bench.json
