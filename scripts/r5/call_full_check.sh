set -e
out=${OUT:?OUT: directory for the results}/r5_full
mkdir -p $out
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -k 10 1500 python3 -m pytest tests -q -x -m gpu > $out/tests_gpu.txt 2>&1 || { tail -40 $out/tests_gpu.txt; exit 1; }
tail -3 $out/tests_gpu.txt
ANNCUR_FUZZ=1 ANNCUR_FUZZ_EXAMPLES=300 timeout -k 10 600 python3 -m pytest tests/test_gpu_random_shapes.py -q -x -m gpu -k "ivf" > $out/fuzz_ivf.txt 2>&1 || { tail -40 $out/fuzz_ivf.txt; exit 1; }
tail -2 $out/fuzz_ivf.txt
timeout -k 10 900 python3 bench.py --full > $out/bench.json 2> $out/bench.err || { tail -30 $out/bench.err; exit 1; }
python3 - $out/bench.json <<'P'
import json, sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
print('ms_per_step', d['ms_per_step'], 'value', d['value'], 'sustained', d.get('sustained',{}).get('ms_per_step'), 'frac', d['roofline']['frac'], 'scan', d.get('roofline_scan',{}).get('achieved'))
iv=d['ivf_search']
for t in ('fp32','bf16'):
    r=iv[t]; print(t, 'search_ms %.3f device %.3f gemm %.3f rest %.3f tile_ratio %.3f frac %.3f' % (r['search_ms'], r['search_device_ms'], r['kernels']['group_gemm_ms'], r['kernels']['scan_and_id_map_ms'], r['kernels']['tile_flops_ratio'], r['kernels']['roofline']['frac']))
P
