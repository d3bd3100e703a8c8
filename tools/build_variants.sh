# Build alternate copies of libmhpc_amd.so with different compile-time tuning flags into
# mhpc_minimal_env_amd/csrc/_build/var/<name>/.
# (flags apply to the fp64 solve kernels and sweep; with ALL32=1 to their fp32 builds as well.
# Every other object is the default build's: the Makefile's VAR= mode, which also puts the
# variant's device assembly through the build's gate)
# usage: bash tools/build_variants.sh name1 "-DFLAG=.." name2 "-DFLAG=.." ...
set -e
C=$(cd "$(dirname "$0")/../mhpc_minimal_env_amd/csrc" && pwd)
make -s -C "$C" -j"${JOBS:-8}" all >/dev/null
while [ $# -ge 2 ]; do
  make -s -C "$C" -j"${JOBS:-8}" VAR="$1" VARFLAGS="$2" ${ALL32:+ALL32=1} all >/dev/null
  shift 2
done
