// The tracking digest's kernels alone (csrc/track_digest.h), compiled for the device only by tests/test_track_digest.py: none of
// them may touch scratch — k_cand_best keeps each lane's list of arg-maxes in LDS for exactly that reason.
#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_digest.h"
