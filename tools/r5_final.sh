#!/bin/bash
# the round's closing run on a GPU box: full GPU test suite, smoke, the default bench line, the bench with the driver's flags, the rocprofv3
# round profile (kernel trace of the bench command + HBM PMC passes) and the decode-stage profile
cd "$(dirname "$0")/.."; export OUT=$(realpath -m "${OUT:-out}"); mkdir -p $OUT
TAG=${1:-r05}
timeout 1500 python -m pytest tests -m gpu -q > $OUT/${TAG}_pytest.log 2>&1; tail -n 4 $OUT/${TAG}_pytest.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 900 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; tail -n1 $OUT/${TAG}_bench.json | cut -c1-300
timeout 600 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench_driver_flags.json 2> $OUT/${TAG}_bench_driver_flags.err; tail -n1 $OUT/${TAG}_bench_driver_flags.json | cut -c1-300
PS_ARGS="--batch 1024" timeout 900 bash tools/prof_round.sh $TAG > $OUT/${TAG}_prof.log 2>&1; sed -n 1,30p $OUT/${TAG}_prof.log | cut -c1-170
timeout 600 bash tools/prof_decode.sh $TAG > $OUT/${TAG}_prof_decode.log 2>&1; head -5 $OUT/${TAG}_prof_decode.log
# the N > 1 launch paths on this one-GPU box (ranks share the device, the two collectives go over gloo): bench.py's own spawner and the
# driver's launcher line
timeout 600 python bench.py --full --gpus 2 --steps 8 --warmup 4 > $OUT/${TAG}_bench_gpus2_self.json 2> $OUT/${TAG}_bench_gpus2_self.err; tail -n1 $OUT/${TAG}_bench_gpus2_self.json | cut -c1-260
timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 8 --warmup 4 > $OUT/${TAG}_bench_gpus2_torchrun.json 2> $OUT/${TAG}_bench_gpus2_torchrun.err; tail -n1 $OUT/${TAG}_bench_gpus2_torchrun.json | cut -c1-260
