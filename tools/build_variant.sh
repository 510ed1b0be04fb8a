#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...]: the engine and the C++ host built with extra compiler flags into
# helib_amd/lib/variants/NAME/ (libhelib_amd.so + libhelib_amd_host.so side by side, rpath $ORIGIN).  Run a
# benchmark against it with   HX_LIB=$PWD/helib_amd/lib/variants/NAME/libhelib_amd.so
#                             HX_HOST_LIB=$PWD/helib_amd/lib/variants/NAME/libhelib_amd_host.so python bench.py ...
# The units are those of helib_amd/build.py; one that does not name any of the macros keeps the default build's object.
set -e
cd "$(dirname "$0")/.."
python -m helib_amd.build --variant "$@"
ls -la helib_amd/lib/variants/$1
