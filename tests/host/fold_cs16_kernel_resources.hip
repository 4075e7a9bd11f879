// The two CS16 instantiations of the fold's step kernel alone, compiled for the device only by tests/test_fold_cs16_kernel_resources.py:
// four-byte samples change the load stage (fold_cs16_staging.h: half as many samples a piece; at radix 16 four pair sums wait in
// registers behind a barrier) and must keep the int8 fold's budget — 128 registers, four waves per SIMD, no spill, no scratch — and its
// LDS (the step kernel's dynamic kStepLdsBytes: the CS16 pieces go through the same two halves of the exchange plane).
#include "../../rtl-sdr-scanner-cpp_amd/csrc/scan_step.h"

template __global__ void ss::k_scan_step<ss::FMT_CS16, false, 2, true, false, ss::kStepFold8>(ss::StepArgs);   // 65536 points, radix 8
template __global__ void ss::k_scan_step<ss::FMT_CS16, false, 2, true, false, ss::kStepFold16>(ss::StepArgs);  // 131072 points, radix 16
