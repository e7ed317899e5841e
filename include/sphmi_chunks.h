/* The chunk partition of the overlapped step, shared by libsphmi.so (which launches by it) and libsphmi_host.so
 * (which exports it as sphmi_step_chunk_edge, so that it can be checked without a GPU). */
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
#endif /* SPHMI_CHUNKS_H */
