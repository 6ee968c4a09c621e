// walk_wide3.hip -- the L2 register-list walks over 384-byte rows in the pair form (the reference's PLAIN walks over deep (d = 96) vectors at
// efs_hnsw of up to 128, final_test.cpp:84): first pass of a compact index over adjacency rows of one pass, or -- the one-register list only --
// two; every other case stays on the run-time-length instances (same LDS layout).  A unit of its own so that the instantiations build in parallel.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

static const WalkEntry kEntries[] = {WALK_REG(0, 24, true, false, 1, false, false), WALK_REG(0, 24, true, false, 1, true, false), WALK_REG(0, 24, true, false, 2, true, false)};
const WalkEntry* walk_wide3_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
