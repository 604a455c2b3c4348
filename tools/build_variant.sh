# builds lib_ab/libkc_NAME.so: the engine with extra compile flags for the counting kernels
# (A/B of compile-time knobs, loaded through KC_LIB).  usage: tools/build_variant.sh NAME "-DKNOB=V ..."
# With UNITS=query only the table-query kernels (kc_query_w.hip) take the flags, e.g.
#   UNITS=query tools/build_variant.sh tpk -DKC_QUERY_TPK   (thread-per-key lookups for W <= 2)
set -e
NAME=$1; FLAGS=$2
P=canonical-k-mer-hash-table_amd
B=lib_ab/build_$NAME
mkdir -p $B
HIPFLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Wno-unused-value $FLAGS"
U=${UNITS:-count}
for w in 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15; do
  /opt/rocm/bin/hipcc $HIPFLAGS -DKC_W=$w -c $P/csrc/kc_${U}_w.hip -o $B/kc_${U}_w$w.o &
  if (( w % 8 == 0 )); then wait; fi
done
wait
COUNT_O="$P/build/kc_count_w*.o"; QUERY_O="$P/build/kc_query_w*.o"
if [ $U = count ]; then COUNT_O="$B/kc_count_w*.o"; else QUERY_O="$B/kc_query_w*.o"; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o lib_ab/libkc_$NAME.so $P/build/kc_tokenize.o $P/build/kc_util.o \
    $P/build/kc_count.o $P/build/kc_skm.o $COUNT_O $P/build/kc_compact_w*.o $QUERY_O $P/build/kc_api.o -lpthread
echo lib_ab/libkc_$NAME.so
