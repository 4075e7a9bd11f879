// The sparse digest's kernels (csrc/track_digest_sparse.h) beside the stand-alone detect launch whose tile the replay runs and the
// candidates' kernel whose body k_ring_best shares, compiled for the device only by tests/test_track_digest_sparse.py: no replay
// instantiation may use more scratch or fewer waves per SIMD than k_detect_fused<21, 21, 16, 256, false> built from the same tree with
// the same flags, k_digest_cols touches no scratch, and k_ring_best costs no more scratch than k_best_blocked with all of its LDS in
// the dynamic region.
#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_digest_sparse.h"

template __global__ void ss::k_detect_fused<21, 21, 16, 256, false>(ss::DetectArgs);
template __global__ void ss::k_digest_tiles<0>(ss::WatchTilesArgs);
template __global__ void ss::k_digest_tiles<3>(ss::WatchTilesArgs);
template __global__ void ss::k_digest_tiles<4>(ss::WatchTilesArgs);
