#!/bin/bash
# usage: tools/pmc_pass.sh <outdir> <counters...> -- <bench args...>   (one rocprofv3 --pmc pass; counters in their own run)
out=$1; shift
ctrs=()
while [ "$1" != "--" ]; do ctrs+=("$1"); shift; done
shift
root=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc "${ctrs[@]}" --kernel-trace -d "$root/$out" -o pmc -- python3 "$root/bench.py" --full "$@" > "$root/$out.log" 2>&1
