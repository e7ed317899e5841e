// What the translation units of the C ABI share (sph_api_edit.hip: particle editing; sph_api.hip: solver lifetime, stages, step, read-back, slab;
// sph_api_analysis.hip: sampling, surfaces, gradients, diagnostics, components, selection): the order contract and the entry checks.
#pragma once
#include "sph_common.h"

// stage progress bits for the order contract of simulationStep()
enum { P_HASH = 1, P_SORT = 2, P_SORTPOST = 4, P_INDEXX = 8, P_INDEXPOST = 16, P_FIND = 32, P_DENSITY = 64, P_FORCES = 128,
       P_PREDICTPOS = 256, P_PREDICTDENS = 512, P_PRESSUREFORCE = 1024 };

#define NEED(s, bits, what)                                                              \
  do {                                                                                   \
    if (!(s)) { sph_set_error("null solver"); return SPH_ERR_INVALID; }                  \
    if (((s)->progress & (bits)) != (bits)) {                                            \
      sph_set_error("%s called before the stage(s) it depends on (simulationStep order, " \
                    "owPhysicsFluidSimulator.cpp:88-113)", what);                        \
      return SPH_ERR_ORDER;                                                              \
    }                                                                                    \
  } while (0)

// (bodies in sph_api.hip)
int sph_d2h(sph_solver* s, void* dst, const void* src, size_t bytes);  // blocking copy to the host on s->stream
int sph_check_finite_state(sph_solver* s);                             // synchronises the stream; SPH_ERR_INVALID once the state has blown up
int sph_slab_finish(sph_solver* s, int32_t counts[4]);
// (bodies in sph_api_analysis.hip)
int sph_grow_scratch(sph_solver* s, SphScratch& b, size_t bytes);  // device buffer b grown to at least `bytes`
// The selection arguments every call that takes them shares: typeMask must be a non-empty set of bits 1..3; region6 (x0, y0, z0,
// x1, y1, z1) may be null (everything: -inf .. +inf) and must not hold a NaN. SPH_ERR_INVALID with "<what>: ..." otherwise.
int sph_fill_selector(SphSelector* sel, const float* region6 /* may be null */, uint32_t typeMask, const char* what);
// SPH_ERR_ORDER unless a labelling / a selection exists and was made on the current state; *labels: the N labels (device)
int sph_labels_current(sph_solver* s, const char* what, const int32_t** labels);
int sph_selection_current(sph_solver* s, const char* what);

// (a rebuild whose particle count is still on its way to the host — sph_slab_rebuild_framed — is finished first)
#define ENTER_RAW(s) do { if (!(s)) { sph_set_error("null solver"); return SPH_ERR_INVALID; } SPH_HIP(hipSetDevice((s)->cfg.device)); } while (0)
#define ENTER(s) do { ENTER_RAW(s); if ((s)->slabRebuildPending) { const int rcf_ = sph_slab_finish((s), nullptr); if (rcf_ != SPH_OK) return rcf_; } } while (0)
