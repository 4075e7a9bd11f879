// The tracked feed's kernels alone (csrc/track_feed.h), compiled for the device only by tests/test_track_feed.py: none of them may
// touch scratch or spill a register.
#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_feed.h"
