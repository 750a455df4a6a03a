// What the other translation units see of the device-resident RegularizationGraph (nrs_rgraph.hip): the a2 driver (nrs_track.hip) and the
// BA windows served by the graph (nrs_engine_winedges.hpp, nrs_engine_embwin.hpp, nrs_dba.hip).  The C ABI is in include/nrs.h.
// No HIP here: nrs_rgraph_host.hpp builds on it.
#pragma once
#include <cstdint>
#include "../../include/nrs.h"

namespace nrs {

// The lists of one GetEdges call: count[row] = the FULL length of the row's list, of which the first min(count, stride) entries stand at
// [row * stride, ..) of col / status / w / d0.  One type for the block on the device and for its copy in the graph's pinned staging
// area (RgListLayout::view, nrs_rgraph_host.hpp); valid until the graph's next GetEdges.
struct RgDeviceLists { int n_rows, stride; const int *count, *col, *status; const float *w, *d0; };

int rg_capacity(const nrs_rgraph* g);
nrs_ctx* rg_context(const nrs_rgraph* g);
int rg_max_cap_per_point(const nrs_rgraph* g);   // the longest GetEdges prefix a call can ask for: the candidates of a row are sorted in LDS

// GetEdges of the listed points (host ids, each in [0, capacity)) into the graph's pinned staging area, read there in place.
// pass_over: one byte per point or null (k_rg_get_edges `skip`).  lists_to_host = false: the lists stay on the device (rg_walk reads
// them there) and only `count` of the view is filled.
int rg_get_edges_staged(nrs_rgraph* g, int32_t n_ids, const int32_t* ids, int32_t cap_per_point, RgDeviceLists* host, const uint8_t* pass_over,
                        bool lists_to_host = true);
// GetEdges of ids a kernel of the caller listed (n_ids ints on the device, each in [0, capacity)), the lists left on the device (the
// BA window's walk reads them there, nrs_engine_winedges.hpp)
int rg_get_edges_device(nrs_rgraph* g, int32_t n_ids, const int32_t* d_ids, int32_t cap_per_point, RgDeviceLists* o);
// The walk of OPT:252-279 over the lists of the last rg_get_edges_staged(.., lists_to_host = false) call.  code: n_map ints
// (nrs_track.hip walk_code); is_node: one byte per row or null (every optimised point a vertex).  Outputs (host): n_acc[n], acc[11 n]
// (indices among the optimised points), acc_w / acc_d0[11 n], ended[n], lost[n_map].  *converged = 0: the passes ran out (the caller
// walks on the host instead).
int rg_walk(nrs_rgraph* g, int n_map, const int* code, const uint8_t* is_node, int* n_acc, int* acc, float* acc_w, float* acc_d0,
            uint8_t* ended, uint8_t* lost, int* converged, int* passes);

}  // namespace nrs
