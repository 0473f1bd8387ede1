# Build a variant of libdcx.so whose dcx_resblock.hip is compiled with extra flags (the other objects
# are the in-tree build's, copied with their time stamps) into distilcodec_nabeel_amd/<name>.so;
# select it with DCX_LIB=...
# Usage: bash tools/build_rp_variant.sh NAME "-DFLAG ..."
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; FLAGS=$2
C=$R/distilcodec_nabeel_amd/csrc
make -C $C -s -j8 >/dev/null
mkdir -p $C/build_$NAME
cp -p $C/build/*.o $C/build_$NAME/
rm -f $C/build_$NAME/dcx_resblock.o
make -C $C -s BUILD=build_$NAME OUT=../$NAME.so EXTRA_RESBLOCK="$FLAGS"
echo built $R/distilcodec_nabeel_amd/$NAME.so
