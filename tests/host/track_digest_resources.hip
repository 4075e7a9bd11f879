// The kernels of csrc/track_digest.h alone (k_window_peaks, k_save_tail), compiled for the device only by tests/test_track_digest.py:
// neither may touch scratch. (The candidates' kernel has tests/host/track_digest_blocked_resources.hip.)
#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_digest.h"
