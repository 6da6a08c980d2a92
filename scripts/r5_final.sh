#!/bin/bash
# round 5's final measurement set (one GPU visit): smoke, -m gpu tests, the bench line (full: cpu baseline, live traffic, other configs), the same under
# rocprofv3 --kernel-trace --stats, decoder per corpus file and on the streams built against it (round-5 kernel vs the round-4 one from the lab
# library), compress by batch size, host API, small blocks, PMC passes of the decoder.
cd "$(dirname "$0")/.."
RES=${RES:-results}     # where this script's logs and lines go
mkdir -p "$RES"; export TMPDIR=/tmp
T=${TAG:-r05zz}
(timeout 200 python __graft_entry__.py smoke > $RES/${T}_smoke.log 2>&1; echo "smoke rc=$?" >> $RES/${T}_smoke.log); tail -2 $RES/${T}_smoke.log
timeout 900 python -m pytest tests -m gpu -q -x > $RES/${T}_pytest.log 2>&1; tail -2 $RES/${T}_pytest.log
timeout 600 python bench.py --full > $RES/${T}_bench_line.json 2> $RES/${T}_bench.err; tail -c 300 $RES/${T}_bench_line.json; echo
rm -rf $RES/${T}_prof
(cd /tmp && BENCH_NO_PLAIN=1 BENCH_NO_DEFAULT_SEARCH=1 timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OLDPWD/$RES/${T}_prof -o bench -- python $OLDPWD/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-live-traffic --no-other-configs > $OLDPWD/$RES/${T}_bench_line_under_rocprof.json 2> $OLDPWD/$RES/${T}_rocprof.err)
f=$(find $RES/${T}_prof -name "*kernel_stats.csv" | head -1); cp "$f" $RES/${T}_bench_kernel_stats.csv; head -5 $RES/${T}_bench_kernel_stats.csv | cut -c1-160
MODES="chains chains_r04" timeout 600 python scripts/decode_by_file.py 32768 2>&1 | grep '"file"' > $RES/${T}_decode_by_file.jsonl; cat $RES/${T}_decode_by_file.jsonl | cut -c1-220
for d in html low mixed; do for m in chains chains_r04; do DATA=$d SNAPPIER_HIP_DECODE=$m REPS=5 timeout 300 python scripts/time_decompress.py 163840 2>&1 | tail -1; done; done > $RES/${T}_decode_new_vs_r04.jsonl; cat $RES/${T}_decode_new_vs_r04.jsonl
for m in chains chains_r04; do SNAPPIER_HIP_DECODE=$m timeout 300 python scripts/adversarial_streams.py 2>&1 | grep -E "^\{"; done > $RES/${T}_adversarial_streams.jsonl; cat $RES/${T}_adversarial_streams.jsonl | cut -c1-200
timeout 900 python scripts/compress_by_batch.py 1024 4096 16383 16384 32768 65536 163840 2>&1 | grep blocks > $RES/${T}_compress_by_batch.jsonl; cat $RES/${T}_compress_by_batch.jsonl
timeout 600 python scripts/host_api_rates.py 65536 4194304 268435456 1073741824 2>&1 | grep bytes > $RES/${T}_host_api.jsonl; cat $RES/${T}_host_api.jsonl
timeout 300 python scripts/small_blocks.py 64 256 1024 4096 2>&1 | grep block_bytes > $RES/${T}_small_blocks.jsonl; cat $RES/${T}_small_blocks.jsonl
EXTRA_PASSES="" MODES="chains chains_r04" timeout 300 bash scripts/r5_pmc_decode.sh > $RES/${T}_pmc_decode.txt 2>&1; grep -c SQ_ $RES/${T}_pmc_decode.txt
