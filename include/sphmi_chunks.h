/* The chunk partition of the overlapped step and the launch order and halo check of the pipelined step (DESIGN.md
 * 32), shared by libsphmi.so (which launches by them) and libsphmi_host.so (which exports them as sphmi_step_chunk_edges,
 * sphmi_step_pipeline_schedule and sphmi_step_halo_check, so that they can be checked without a GPU). */
#ifndef SPHMI_CHUNKS_H
#define SPHMI_CHUNKS_H
#include <stdint.h>

#define SPH_CHUNK_ALIGN 256 /* == SPH_BLOCK: a multiple of findNeighbors' 128-particle workgroup and of the 64-particle map tile */

/* Edge i (0 .. chunks) of the partition of the sorted particles [0, n) into `chunks` ranges [edge i, edge i + 1): the
 * ceil(n / 256) blocks of 256 particles dealt as evenly as whole blocks allow. Edge 0 is 0, edge `chunks` is n, every edge in
 * between is a multiple of 256 below n; with more chunks than blocks some ranges are empty. */
static inline int64_t sphChunkEdge(int64_t n, int32_t chunks, int32_t i) {
  if (n <= 0 || chunks <= 0 || i <= 0) return 0;
  if (i >= chunks) return n;
  const int64_t blocks = (n + SPH_CHUNK_ALIGN - 1) / SPH_CHUNK_ALIGN;
  return (blocks * i / chunks) * SPH_CHUNK_ALIGN;
}

/* ---- the pipelined step. Stage 0 of a chunk is its density pass and record pack (behind its findNeighbors
 * launch); stage 1 the forces kernel; stages 2i + 1 (i >= 1) and 2i + 2 the predicted density and the pressure force of
 * predict-correct iteration i (iteration 0's predicted density is part of the forces kernel). */
#define SPH_PIPELINE_STAGES_MAX 6
#define SPH_PIPELINE_ITEMS_MAX(chunks) ((chunks) * (SPH_PIPELINE_STAGES_MAX + 1))
#ifdef __HIPCC__
#define SPH_CHUNKS_FN __host__ __device__ static inline
#else
#define SPH_CHUNKS_FN static inline
#endif

/* The depth a step takes when `depth` stages are asked for: no more than the step has (2 * maxIteration), and only the forces
 * kernel with elastic matter (k_elastic and the membrane kernels sit between the later stages and read arbitrary particles). */
static inline int32_t sphPipelineDepth(int32_t depth, int32_t maxIteration, int32_t hasElastic) {
  int32_t d = depth < 0 ? 0 : depth;
  if (d > SPH_PIPELINE_STAGES_MAX) d = SPH_PIPELINE_STAGES_MAX;
  if (d > 2 * maxIteration) d = maxIteration > 0 ? 2 * maxIteration : 0;
  if (hasElastic && d > 1) d = 1;
  return d;
}

/* The launches of the chunk stream in issue order: for every step t = 0 .. chunks - 1 + D stage 0 of chunk t, then stage k of
 * chunk t - k for k = 1 .. D (each only for a chunk in [0, chunks)), D being the clamped depth. So stage k of chunk c is issued
 * one step after stage k - 1 of chunk c + 1. Writes stage[i], chunk[i] and returns the count (<= SPH_PIPELINE_ITEMS_MAX). */
static inline int32_t sphPipelineSchedule(int32_t chunks, int32_t depth, int32_t maxIteration, int32_t hasElastic, int32_t* stage,
                                          int32_t* chunk) {
  const int32_t D = sphPipelineDepth(depth, maxIteration, hasElastic);
  int32_t n = 0;
  for (int32_t t = 0; t < chunks + D; t++)
    for (int32_t k = 0; k <= D; k++) {
      const int32_t c = t - k;
      if (c < 0 || c >= chunks) continue;
      stage[n] = k; chunk[n] = c; n++;
    }
  return n;
}

/* ---- the deferred band scatter. Under the premise of the halo check below, findNeighbors of chunk c reads band
 * records only of particles of chunks c - 1 .. c + 1. The prelude scatters the records of the chunks [0, sphBandDeferFirst); the
 * search launches of the chunks c with c + 1 < sphBandDeferFirst need no others and start at the fork; the records of the chunks
 * from sphBandDeferFirst on are scattered beside them, and every later search launch is issued behind that scatter. With three
 * chunks or fewer nothing is deferred and the function returns `chunks`.
 * 2: chunk 0 alone starts at the fork (measured against 3, profiles/r39/README.md). */
static inline int32_t sphBandDeferFirst(int32_t chunks) { return chunks > 3 ? 2 : chunks; }

/* The halo check of chunk [lo, hi) of the sorted particles: 1 only if every particle that findNeighbors can give a particle of
 * the chunk as a neighbour has its sorted index in [below, above) (the pipelined step: below = edge c - 1, above = edge c + 2).
 * The search looks at cells whose id differs from the particle's by at most reach = gx * gy + gx + 1, and wraps an id below 0 to
 * id + G and one from G on to id - G; keys are sorted, so the chunk's cells lie in [keys[lo], keys[hi - 1]]. cellStart has G + 1
 * entries, [G] = n. A key outside the table (a blown-up state) fails; every table index is inside [0, G]. */
SPH_CHUNKS_FN int sphChunkHaloOk(const uint32_t* keys, const uint32_t* cellStart, int64_t G, int64_t reach, int64_t n, int64_t lo,
                                 int64_t hi, int64_t below, int64_t above) {
  if (hi <= lo) return 1;
  const int64_t kf = keys[lo], kl = keys[hi - 1];
  if (kl >= G || kf > kl) return 0;
  if (kf >= reach) {
    if ((int64_t)cellStart[kf - reach] < below) return 0;
  } else {  /* cells from 0 on, and the wrapped cells kf - reach + G .. G - 1 */
    if (below != 0) return 0;
    const int64_t w = kf - reach + G;
    const int64_t first = (int64_t)cellStart[w < 0 ? 0 : w];
    if (first < n && above < n) return 0;
  }
  if (kl + reach + 1 <= G) {
    if ((int64_t)cellStart[kl + reach + 1] > above) return 0;
  } else {  /* cells up to G - 1, and the wrapped cells 0 .. kl + reach - G */
    if (above != n) return 0;
    const int64_t w = kl + reach + 1 - G;
    const int64_t end = (int64_t)cellStart[w > G ? G : w];
    if (end > 0 && below > 0) return 0;
  }
  return 1;
}
#endif /* SPHMI_CHUNKS_H */
