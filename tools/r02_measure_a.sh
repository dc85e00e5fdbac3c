#!/bin/bash
# Round-2 measurement set A (run on the GPU box through gpurun): bench line, rocprofv3 summary of the same command, PMC traffic.
O=$GRAFT_REPO_ROOT/gpurun_out/r02; mkdir -p $O
cd $GRAFT_REPO_ROOT
python bench.py --full > $O/bench_n1.json 2> $O/bench_n1.err; echo "bench rc $?"; tail -c 300 $O/bench_n1.json
python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline > $O/bench_torchrun_n1.json 2> $O/bench_torchrun_n1.err; echo "torchrun rc $?"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_bench -o b --output-format csv -- python3 $GRAFT_REPO_ROOT/bench.py --steps 10 --warmup 2 --no-cpu-baseline > $O/bench_profiled.json 2> $O/bench_profiled.err; echo "rocprof bench rc $?"
cd $GRAFT_REPO_ROOT && python tools/pmc_traffic.py --out $O/pmc_latest.json > $O/pmc_traffic.log 2>&1; echo "pmc rc $?"; tail -c 400 $O/pmc_traffic.log
python tools/config_timings.py > $O/collector_timings.log 2>&1; echo "timings rc $?"
python tools/emit_probe.py ca13_XL 163000000 4 > $O/emit_probe.log 2>&1
