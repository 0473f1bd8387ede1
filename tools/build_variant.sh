# Build a variant of libdcx.so with extra compile flags into distilcodec_nabeel_amd/<name>.so
# (select it at run time with DCX_LIB=...).  Usage: bash tools/build_variant.sh NAME "-DFLAG ..."
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; FLAGS=$2
make -C $R/distilcodec_nabeel_amd/csrc -s -j8 BUILD=build_$NAME OUT=../$NAME.so EXTRA="$FLAGS"
echo built $R/distilcodec_nabeel_amd/$NAME.so
