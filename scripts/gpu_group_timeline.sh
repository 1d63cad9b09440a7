# usage: bash scripts/gpu_group_timeline.sh <tag> <output folder> : who waits for whom in the keypoint stage of one overlapped bench step (B = 64).
# Two profiler runs of the same command (HESAFF_AMD_LIB chooses the library, as everywhere): a kernel trace alone, and a kernel trace
# together with the HIP runtime API trace, which adds the moment the host submitted every launch and the host calls that lasted long.
# Leaves <output folder>/gt_<tag>/group_timeline_kernels_only.txt, group_timeline_with_api.txt and timeline_1ms.txt.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
[ $# -ge 2 ] || { echo "usage: $0 <tag> <output folder>" >&2; exit 2; }
mkdir -p "$2" && O=$(cd "$2" && pwd)/gt_$1
mkdir -p $O
BENCH="python3 $R/bench.py --gpus 1 --steps 1 --warmup 1 --batch ${BATCH:-64}"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $O/kt -o p -- $BENCH > $O/kt_bench.txt 2>&1 || exit 1
KT=$(find $O/kt -name "*kernel_trace.csv" | head -1)
python3 $R/scripts/group_timeline.py $KT > $O/group_timeline_kernels_only.txt || exit 1
python3 $R/scripts/timeline.py $KT 1 > $O/timeline_1ms.txt || exit 1
timeout -k 10 240 rocprofv3 --kernel-trace --hip-runtime-trace --output-format csv -d $O/api -o p -- $BENCH > $O/api_bench.txt 2>&1 || exit 1
python3 $R/scripts/group_timeline.py $(find $O/api -name "*kernel_trace.csv" | head -1) $(find $O/api -name "*hip_api_trace.csv" | head -1) > $O/group_timeline_with_api.txt || exit 1
find $O -name "*.csv" -delete; find $O -name "*.db" -delete
