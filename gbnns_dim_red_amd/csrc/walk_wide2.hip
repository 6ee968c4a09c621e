// walk_wide2.hip -- the L2 two-list walks over 384- and 512-byte rows in the pair form (the reference's PLAIN walks over deep (d = 96) and
// sift (d = 128) vectors at efs_hnsw of more than 128, final_test.cpp:84); a unit of its own so that the instantiations build in parallel.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

static const WalkEntry kEntries[] = {WALK_BIG_SET(0, 24), WALK_BIG_LATE(24), WALK_BIG_SET(0, 32), WALK_BIG_LATE(32)};
const WalkEntry* walk_wide2_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
