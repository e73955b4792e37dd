// The option keys' names for the library's own host code: get_option /
// set_option (rse_kernels.hpp) are called with RSE_OPT_* names only.  The
// table behind them is kOptionRows in rse_kernels.hip.
#pragma once

#include "../../include/rse_hip.h"
#include "../../include/rse_hip_tune.h"

// -DRSE_TUNE_SPLITS builds only (make tune), so not in the public headers:
// wide modules built without their barriers, for timing (wrong bytes).
#define RSE_OPT_TUNE_NOSYNC 47

namespace rse {
// Whether rse_set_option takes the key without RSE_TUNE=1 in the environment
// (include/rse_hip.h's keys; the tuning switches of rse_hip_tune.h need it).
bool caller_may_set_option(int key);
}  // namespace rse
