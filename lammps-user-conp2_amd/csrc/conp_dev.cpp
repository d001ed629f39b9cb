// The two process-wide objects of conp_dev.hpp, defined in this translation unit only: a second definition is a link error.
#include "conp_dev.hpp"

namespace conp::dev {
std::string &last_error() { thread_local std::string e; return e; }
GuardZones &GuardZones::get() { static GuardZones g; return g; }
}  // namespace conp::dev
