// The blocked candidates' kernel alone (csrc/track_digest_blocked.h; it brings csrc/track_digest.h's kernels with it), compiled for
// the device only by tests/test_track_digest_blocked.py: k_best_blocked may not touch scratch — tables and lists live in LDS.
#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_digest_blocked.h"
