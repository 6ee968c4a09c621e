// walk_wide.hip -- the L2 walks over 192-, 256- and 576-byte rows (d_low = 48 / 64 / 144: the reference's deep row, the GIST shape, the
// reference's glove row).  576-byte rows have the pair form in the two-list kernels (2 x 72 registers of row and query); their shorter
// beams take the run-time-length instances of walk_l2.hip.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

static const WalkEntry kEntries[] = {
    WALK_GENERIC_SET(0, 12), WALK_WIDE(12, false), WALK_WIDE(12, true),
    WALK_GENERIC_SET(0, 16), WALK_WIDE(16, false), WALK_WIDE(16, true),
    WALK_LDS_SET(0, 36), WALK_BIG_SET(0, 36), WALK_BIG_LATE(36),
};
const WalkEntry* walk_wide_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
