#!/bin/bash
# Builds the library from another git revision into sparkfm_amd/lib/libfmhip_<name>.so (A/B runs on one
# GPU box: FMHIP_LIB=sparkfm_amd/lib/libfmhip_<name>.so python tools/ab_bench.py ...).
#   tools/build_variant.sh <name> [git-rev, default HEAD; WORK = the working tree]
#   EXTRA_FLAGS="-DFOO=1" adds compiler flags (experiment macros)
# The revision's own sparkfm_amd/_build.py says which translation units it has and which flags they take.
set -e
name=$1; rev=${2:-HEAD}
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d /tmp/fmhip_variant.XXXXXX)
trap 'rm -rf $tmp' EXIT
if [ "$rev" = WORK ]; then
  mkdir -p $tmp/sparkfm_amd
  cp -r $root/include $tmp/include
  cp -r $root/sparkfm_amd/csrc $root/sparkfm_amd/_build.py $tmp/sparkfm_amd/
else
  git -C $root archive $rev sparkfm_amd/_build.py sparkfm_amd/csrc include | tar -x -C $tmp
fi
query() { python3 -c "import sys; sys.path.insert(0, '$tmp/sparkfm_amd'); import _build; print(' '.join(_build.$1))"; }
sources=$(query HIP_SOURCES); flags=$(query HIPCC_FLAGS)
objs=""; pids=""
for f in $sources; do
  /opt/rocm/bin/hipcc $flags ${EXTRA_FLAGS:+-DFMHIP_ABLATION_BUILD} $EXTRA_FLAGS -c $tmp/sparkfm_amd/csrc/$f -o $tmp/${f%.*}.o &
  pids="$pids $!"
  objs="$objs $tmp/${f%.*}.o"
done
for p in $pids; do wait $p; done
mkdir -p $root/sparkfm_amd/lib
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/sparkfm_amd/lib/libfmhip_$name.so $objs -Wl,-rpath,/opt/rocm/lib -lpthread -ldl
echo $root/sparkfm_amd/lib/libfmhip_$name.so
