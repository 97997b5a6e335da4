#!/bin/bash
# One GPU session: microbench, GPU tests, bench, rocprof kernel trace.
# Every GPU step has its own time limit; a crash/abort/timeout stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
ok_or_stop() {  # $1 = exit code, $2 = step; test failures (1) continue, faults stop
  case "$1" in
    0|1) return 0 ;;
    *) echo "STOP after $2 (exit $1)"; exit "$1" ;;
  esac
}
STEPS="${STEPS:-ubench tests bench prof}"
# the steps below read the whole line (host paths, per-kernel times, side configs)
BENCH_ARGS="--full ${BENCH_ARGS:-}"
C5_ARGS="--full ${C5_ARGS:-}"
for s in $STEPS; do
  case "$s" in
    ubench) timeout -k 10 120 bdls_amd/lib/ubench > gpurun_out/ubench.json 2> gpurun_out/ubench.err; rc=$?; cat gpurun_out/ubench.json; ok_or_stop $rc ubench ;;
    tests)  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread ${TEST_ARGS:-} > gpurun_out/pytest_gpu.log 2>&1; rc=$?; tail -5 gpurun_out/pytest_gpu.log; ok_or_stop $rc tests ;;
    smoke)  timeout -k 10 300 python -u __graft_entry__.py > gpurun_out/smoke.log 2>&1; rc=$?; tail -2 gpurun_out/smoke.log; ok_or_stop $rc smoke ;;
    lat)    for c in 3 4; do timeout -k 10 300 python -u bench.py --config $c --steps ${LAT_STEPS:-30} --warmup 3 > gpurun_out/lat$c.json 2> gpurun_out/lat$c.err; rc=$?; cat gpurun_out/lat$c.json; tail -3 gpurun_out/lat$c.err; case $rc in 0|3) ;; *) echo "STOP after lat$c (exit $rc)"; exit $rc ;; esac; done ;;
    hostinfo) (nproc; python -c "import os; print(os.cpu_count(), len(os.sched_getaffinity(0)))"; cat /sys/fs/cgroup/cpu.max 2>/dev/null; lscpu | head -20) > gpurun_out/hostinfo.txt 2>&1; cat gpurun_out/hostinfo.txt ;;
    bench)  timeout -k 10 600 python bench.py ${BENCH_ARGS:-} > gpurun_out/bench.json 2> gpurun_out/bench.err; rc=$?; cat gpurun_out/bench.json; tail -3 gpurun_out/bench.err; ok_or_stop $rc bench ;;
    prof)   export TMPDIR=/tmp; timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/prof -o run -- python3 bench.py --gpus 1 --steps 20 --warmup 5 ${BENCH_ARGS:-} > gpurun_out/prof_bench.json 2> gpurun_out/prof.log; rc=$?; tail -3 gpurun_out/prof.log; ok_or_stop $rc prof; python3 tools/prof_check.py gpurun_out/prof/run_kernel_trace.csv gpurun_out/prof_bench.json gpurun_out/prof_check.json ;;
    exp)    for pass in $(seq ${EXP_PASSES:-2}); do for so in bdls_amd/lib/libbdlship.so exp/libbdlship_*.so; do v=$(basename $so .so); BDLS_HIP_LIB=$PWD/$so timeout -k 10 300 python bench.py --steps ${EXP_STEPS:-20} --warmup 3 --cpu-baseline 0 --side-configs 0 ${BENCH_ARGS:-} > gpurun_out/exp_${v}_p$pass.json 2> gpurun_out/exp_${v}_p$pass.err; rc=$?; echo "$v pass $pass rc=$rc"; case $rc in 0|3) ;; *) echo "STOP after exp $v (exit $rc)"; exit $rc ;; esac; done; done ;;
    c5)     # config 5 at one GPU: the whole seeded 64M unique-key batch (VERDICT r4 missing #1);
            # C5_RUNS=2 runs it twice, the second reading the shard from the disk cache
            for run in $(seq ${C5_RUNS:-1}); do timeout -k 10 ${C5_TIMEOUT:-900} python -u bench.py --config 5 --gpus 1 --steps ${C5_STEPS:-3} --warmup 1 ${C5_ARGS:-} > gpurun_out/bench_c5_run$run.json 2> gpurun_out/bench_c5_run$run.err; rc=$?; cat gpurun_out/bench_c5_run$run.json; tail -3 gpurun_out/bench_c5_run$run.err; case $rc in 0|3) ;; *) echo "STOP after c5 run $run (exit $rc)"; exit $rc ;; esac; done ;;
    lanes1) BH_LANES=1 timeout -k 10 600 python bench.py --steps ${EXP_STEPS:-20} --warmup 2 --cpu-baseline 0 --side-configs 0 ${BENCH_ARGS:-} > gpurun_out/bench_lanes1.json 2> gpurun_out/bench_lanes1.err; rc=$?; cat gpurun_out/bench_lanes1.json; ok_or_stop $rc lanes1 ;;
    nostagger) BH_LANE_STAGGER=0 timeout -k 10 600 python bench.py --steps ${EXP_STEPS:-20} --warmup 2 --cpu-baseline 0 --side-configs 0 ${BENCH_ARGS:-} > gpurun_out/bench_nostagger.json 2> gpurun_out/bench_nostagger.err; rc=$?; cat gpurun_out/bench_nostagger.json; ok_or_stop $rc nostagger ;;
    noll) BH_LL=0 timeout -k 10 600 python bench.py --steps ${EXP_STEPS:-20} --warmup 2 --cpu-baseline 0 --side-configs 0 ${BENCH_ARGS:-} > gpurun_out/bench_noll.json 2> gpurun_out/bench_noll.err; rc=$?; cat gpurun_out/bench_noll.json; ok_or_stop $rc noll ;;
    probe)  timeout -k 10 180 python -u tools/small_probe.py 1 8 64 256 > gpurun_out/small_probe.json 2> gpurun_out/small_probe.err; rc=$?; cat gpurun_out/small_probe.json; ok_or_stop $rc probe ;;
    probeprof) export TMPDIR=/tmp; timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/prof_small -o small -- python3 tools/small_probe.py 1 64 > gpurun_out/probeprof.log 2>&1; rc=$?; tail -2 gpurun_out/probeprof.log; ok_or_stop $rc probeprof ;;
    pmclist) export TMPDIR=/tmp; timeout -k 10 120 rocprofv3 -L > gpurun_out/pmc_list.txt 2>&1; rc=$?; ok_or_stop $rc pmclist ;;
    pmc)    export TMPDIR=/tmp
            for grp in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES GRBM_GUI_ACTIVE" "SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES" "FETCH_SIZE" "WRITE_SIZE"; do
              tag=$(echo $grp | tr ' ' '_' | cut -c1-40)
              # one compute lane: each kernel alone on the device, so GRBM_GUI_ACTIVE is its own
              BH_LANES=1 timeout -k 10 600 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d gpurun_out/pmc_$tag -o pmc -- python3 bench.py --steps 1 --warmup 0 --cpu-baseline 0 --hbm-resident 0 --side-configs 0 ${BENCH_ARGS:-} > gpurun_out/pmc_$tag.log 2>&1; rc=$?; ok_or_stop $rc "pmc $grp"
            done ;;
  esac
done
echo DONE
