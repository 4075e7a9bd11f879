// The headline kernel's CS16 instantiation alone, compiled for the device only by tests/test_cs16_kernel_resources.py: 16-bit complex
// input takes CF32's path and differs from it in the frame load alone, so it keeps CF32's register budget (512 threads x 64 VGPRs =
// four workgroups per CU whatever their roles) and CF32's scratch-free frame path.
#include "../../rtl-sdr-scanner-cpp_amd/csrc/scan_step.h"

template __global__ void ss::k_scan_step<ss::FMT_CS16, false, 2, true, false, 0>(ss::StepArgs);  // 8192 points, CS16, no spectrogram branch
