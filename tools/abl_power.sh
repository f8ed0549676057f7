# the power-limit test: the grouped conv launch and its MFMA-only / load-only variants (ABL_ONE=5 / 6) on random vs all-zero operands.
# The variants need a -DPOPCORN_CONV_ABLATE build (tools/build_variant.sh ablate -DPOPCORN_CONV_ABLATE; POPCORN_HIP_LIB=ab/libpopcorn_ablate.so
# in front of this script); a product build prints the full rows only.
for z in "" 1 "" 1; do for d in 0 5 6; do ABL_ZERO=$z ABL_ONE=$d python3 tools/ablate_conv_group.py 8 8 128 | tail -1 | sed "s/^/zero=[$z] /"; done; done
