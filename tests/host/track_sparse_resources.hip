// The sparse tracked feed's kernels (csrc/track_sparse.h) beside the stand-alone detect launch whose tile k_watch_tiles runs, compiled
// for the device only by tests/test_track_sparse.py: the replay may use no more scratch and no fewer waves per SIMD than
// k_detect_fused<21, 21, 16, 256, false> built from the same tree with the same flags.
#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_sparse.h"

template __global__ void ss::k_detect_fused<21, 21, 16, 256, false>(ss::DetectArgs);
