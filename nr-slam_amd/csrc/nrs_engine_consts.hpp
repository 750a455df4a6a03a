// Constants of the engine's interface that host-only code shares with it (no HIP here: nrs_nd_prep_host.hpp, nrs_kft_prep_host.hpp,
// nrs_devpack_host.hpp and their stand-alone checks compile with a plain C++ compiler).
#pragma once
#include <cstdint>

namespace nrs {

enum : uint8_t { RF_OBS = 1, RF_REPROJ_ACTIVE = 2, RF_FIXED = 4 };   // EngineSpec::rflag
constexpr int ROW_ALIGN = 256;       // pose row padding; also rows per k_reproj workgroup
constexpr int BLK = 256;             // threads per workgroup everywhere
constexpr int SK_MAX = 11;           // embedded mode (nrs_engine_skin.hpp): nodes per skinned observation (the walk of OPT:255-279 accepts 11)
// keyframe-block factorisation (nrs_engine_kft.hpp; set-up stages: nrs_kft_prep_host.hpp)
constexpr int KFT_B = 64;            // pivot block / tile of the sweeps
constexpr int KFT_TC = 4;            // columns of S_to a k_kft_tgt workgroup stages in LDS (KFT_TC rows of ld doubles)
constexpr uint32_t KFT_BD = 0x40000000u;   // te_src: the value is bd_val[index] (pe_src: type 3)

}  // namespace nrs
