// Constants of the engine's interface that host-only code shares with it (no HIP here: nrs_nd_prep_host.hpp and its stand-alone check
// compile with a plain C++ compiler).
#pragma once
#include <cstdint>

namespace nrs {

enum : uint8_t { RF_OBS = 1, RF_REPROJ_ACTIVE = 2, RF_FIXED = 4 };   // EngineSpec::rflag
constexpr int SK_MAX = 11;           // embedded mode (nrs_engine_skin.hpp): nodes per skinned observation (the walk of OPT:255-279 accepts 11)

}  // namespace nrs
