// walk_dot.hip -- the generic walks with the negative-dot metric (Angular::Dist): 128-byte rows in the pair form, and run-time length.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

static const WalkEntry kEntries[] = {
    WALK_GENERIC_SET(1, 8),
    WALK_GENERIC_SET(1, 0),
};
const WalkEntry* walk_dot_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
