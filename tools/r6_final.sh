#!/bin/bash
# the round's closing run on one GPU box: full GPU test suite, smoke, the default bench line, the bench with the driver's flags, then the
# rocprofv3 evidence for every configuration of the line (tools/r6_profiles.sh)
cd "$(dirname "$0")/.."; export OUT=$(realpath -m "${OUT:-out}"); mkdir -p $OUT
TAG=${1:-r06}
timeout 1500 python -m pytest tests -m gpu -q > $OUT/${TAG}_pytest.log 2>&1; tail -n 4 $OUT/${TAG}_pytest.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 900 python bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err; tail -n1 $OUT/${TAG}_bench_default.json | cut -c1-300
timeout 600 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench_driver_flags.json 2> $OUT/${TAG}_bench_driver_flags.err; tail -n1 $OUT/${TAG}_bench_driver_flags.json | cut -c1-300
timeout 1800 bash tools/r6_profiles.sh $TAG > $OUT/${TAG}_profiles.log 2>&1; grep -c "" $OUT/${TAG}_profiles.log
