#!/bin/bash
# usage: bash profiles/build_variant.sh NAME "EXTRA FLAGS" [file.hip ...]
# A/B builds of edited kernels.  Builds attention-gan_amd/csrc/variants/libagan_NAME.so: the shipped objects with the listed sources (default
# conv_p16.hip) recompiled as they stand in the tree, EXTRA FLAGS (may be "") appended -- to time an edited kernel against the shipped library in
# one process each, `AGAN_LIB=.../variants/libagan_NAME.so python profiles/conv_micro.py ...` (never shipped).
# The source list, the compile and link lines and the per-file flags are csrc/Makefile's own (`make -n` prints its recipes).
set -e -o pipefail
NAME=$1; FLAGS=$2; shift 2 || true
VARIANT_SRCS=${@:-conv_p16.hip}
cd "$(dirname "$0")/../attention-gan_amd/csrc"
SRCS=$(sed -n 's/^SRCS := //p' Makefile)
make -j8 > /dev/null   # the shared objects must be current (headers change struct layouts)
mkdir -p variants
RECIPES=$(make -n -B libagan_hip.so)
LINK=$(tail -n 1 <<< "$RECIPES")
LINK=${LINK/-o libagan_hip.so/-o variants/libagan_$NAME.so}
for s in $VARIANT_SRCS; do
  o=${s%.hip}
  echo " $SRCS " | grep -q " $s " || { echo "$s is not in the Makefile's SRCS" >&2; exit 1; }
  COMPILE=$(grep -- " -c $s -o $o.o" <<< "$RECIPES")
  # (hipcc names a compilation unit's device symbols after a hash of its whole command line, `-o` included: the variant is compiled under the
  #  Makefile's own object name, the shipped object set aside meanwhile, so that an unchanged source with no extra flags gives the shipped code object)
  mv $o.o variants/$o.shipped.o
  trap "mv variants/$o.shipped.o $o.o" EXIT
  eval "${COMPILE/ -o $o.o/ $FLAGS -o $o.o}"
  mv $o.o variants/${o}_$NAME.o
  mv variants/$o.shipped.o $o.o
  trap - EXIT
  LINK=${LINK/ $o.o/ variants/${o}_$NAME.o}
done
eval "$LINK"
rm -f variants/*_$NAME.o
echo built variants/libagan_$NAME.so
